"""Stage E of the people assembly (dedupe) restated in float64 loops: the rule of include/deepcut_hip.h, dc_dedupe_params, step by step.

PARITY UNPINNED BY THE REFERENCE: the reference stops at the maps; the rule is this project's own and this file is its second statement.
Plain Python floats (IEEE doubles), one operation per line of the rule, sums over the joints ascending.  Besides the result it returns
a record of every pair (A ranked before B) — n_c, D, the decision, the ranks, whether the sweep consulted it — and the smallest
|D - max_dist| / max(max_dist, tiny) over the pairs with n_c >= min_common: the device may contract multiply-adds, so a scene is a
fair test of the decisions only when that margin is far above (2J + 4) * 2^-53, or the pair is an intended exact tie."""
import math

import numpy as np

TINY = float(np.finfo(np.float64).tiny)
INF = float("inf")


def _fmin(a, b):  # C's fmin: a NaN operand is passed over
    if a != a:
        return b
    if b != b:
        return a
    return a if a < b else b


def _fmax(a, b):
    if a != a:
        return b
    if b != b:
        return a
    return a if a > b else b


def dedupe_ref(people, cand=None, max_dist=0.05, min_common=3, min_size=32.0, sigma=None, absorb=True):
    """people: [n, J, 3] float64 (x, y, score), cand: int [n, J] or None (assigned == held: 0 where held, -1 elsewhere).
    -> dict: "people" [m, J, 3], "cand" int32 [m, J], "kept_from" int32 [m], "suppressed_by" int32 [n] (input index or -1), "rank"
    int [n] (rank of every input person), "pairs": list of (a, b, rank_a, rank_b, n_c, D, similar, consulted) with a ranked before b
    (input indices), "margin": float (inf when no pair has n_c >= min_common)."""
    ppl = np.asarray(people, np.float64)
    n, J = ppl.shape[:2]
    P = [[(float(ppl[q, j, 0]), float(ppl[q, j, 1]), float(ppl[q, j, 2])) for j in range(J)] for q in range(n)]
    sig2 = [1.0] * J if sigma is None else [float(s) * float(s) for s in np.asarray(sigma, np.float64).reshape(J)]
    max_dist, min_size = float(max_dist), float(min_size)

    # 1. held, score, size
    held = [[P[q][j][2] > 0.0 for j in range(J)] for q in range(n)]
    if cand is None:
        cnd = [[0 if held[q][j] else -1 for j in range(J)] for q in range(n)]
    else:
        c = np.asarray(cand).reshape(n, J)
        cnd = [[int(c[q, j]) for j in range(J)] for q in range(n)]
    S, s2 = [], []
    for q in range(n):
        total = 0.0
        x0, x1, y0, y1 = INF, -INF, INF, -INF
        for j in range(J):
            if held[q][j]:
                x, y, sc = P[q][j]
                total += sc
                x0, x1, y0, y1 = _fmin(x0, x), _fmax(x1, x), _fmin(y0, y), _fmax(y1, y)
        s = min_size
        if x1 >= x0:
            s = _fmax(s, _fmax(x1 - x0, y1 - y0))
        S.append(total)
        s2.append(s * s)

    # 2. rank
    order = sorted(range(n), key=lambda q: (-S[q], q))  # S is never a NaN; -inf sorts first
    rank = [0] * n
    for r, q in enumerate(order):
        rank[q] = r

    # 3. distance of every pair, A ranked before B
    def dist(a, b):
        total, nc = 0.0, 0
        for j in range(J):
            if held[a][j] and held[b][j]:
                dx = P[a][j][0] - P[b][j][0]
                dy = P[a][j][1] - P[b][j][1]
                num, den = dx * dx + dy * dy, s2[a] * sig2[j]
                total += float(np.float64(num) / np.float64(den)) if den == 0.0 else num / den  # Python raises where IEEE gives inf / NaN
                nc += 1
        if nc == 0:
            return 0, float("nan")
        return nc, total / nc

    pair = {}
    margin = INF
    with np.errstate(all="ignore"):
        for ra in range(n):
            for rb in range(ra + 1, n):
                a, b = order[ra], order[rb]
                nc, D = dist(a, b)
                similar = nc >= min_common and D <= max_dist  # False for a NaN
                pair[(ra, rb)] = [a, b, ra, rb, nc, D, bool(similar), False]
                if nc >= min_common and D == D:
                    gap = abs(D - max_dist) / max(max_dist, TINY) if not math.isinf(D) else INF
                    margin = min(margin, gap)

    # 4. sweep in rank order
    by = [-1] * n  # by input index: the input index of the kept person that suppressed it
    kept_ranks = []
    for rb in range(n):
        b = order[rb]
        for ra in kept_ranks:
            rec = pair[(ra, rb)]
            rec[7] = True
            if rec[6]:
                by[b] = order[ra]
                break
        else:
            kept_ranks.append(rb)

    # 5. absorb, 6. compaction in input order
    kept = [q for q in range(n) if by[q] < 0]
    out = np.zeros((len(kept), J, 3), np.float64)
    out_c = np.full((len(kept), J), -1, np.int32)
    for o, a in enumerate(kept):
        donors = sorted((q for q in range(n) if by[q] == a), key=lambda q: rank[q])
        for j in range(J):
            src, c = a, cnd[a][j]
            if absorb and c < 0:
                for d in donors:
                    if cnd[d][j] >= 0:
                        src, c = d, cnd[d][j]
                        break
            out[o, j] = ppl[src, j]
            out_c[o, j] = c
    return {"people": out, "cand": out_c, "kept_from": np.array(kept, np.int32).reshape(-1), "suppressed_by": np.array(by, np.int32).reshape(-1),
            "rank": rank, "pairs": [tuple(v) for v in pair.values()], "margin": margin}


def dedupe_ref_batch(people, n_people, cand=None, **params):
    """people [nb, P, J, 3], n_people [nb], cand [nb, P, J] or None -> (n_out [nb], people_out [nb, P, J, 3], cand_out [nb, P, J],
    kept_from [nb, P], suppressed_by [nb, P], records): the arrays as dc_dedupe_people pads them, records = dedupe_ref's dicts."""
    ppl = np.asarray(people, np.float64)
    nb, P, J = ppl.shape[:3]
    n_out = np.zeros(nb, np.int32)
    out, out_c = np.zeros((nb, P, J, 3), np.float64), np.full((nb, P, J), -1, np.int32)
    kept_from, by = np.full((nb, P), -1, np.int32), np.full((nb, P), -1, np.int32)
    recs = []
    for b in range(nb):
        n = int(n_people[b])
        r = dedupe_ref(ppl[b, :n], None if cand is None else np.asarray(cand)[b, :n], **params)
        m = r["people"].shape[0]
        n_out[b] = m
        out[b, :m], out_c[b, :m], kept_from[b, :m], by[b, :n] = r["people"], r["cand"], r["kept_from"], r["suppressed_by"]
        recs.append(r)
    return n_out, out, out_c, kept_from, by, recs


def all_distances(people, min_common, min_size, sigma=None):
    """The D of every pair with n_c >= min_common that is not a NaN, sorted ascending: what a test picks a max_dist between."""
    r = dedupe_ref(people, None, max_dist=0.0, min_common=min_common, min_size=min_size, sigma=sigma, absorb=False)
    return sorted(p[5] for p in r["pairs"] if p[4] >= min_common and p[5] == p[5])


def check_margins(rec, max_dist, min_common, exact=None, least=1e-9):
    """The condition on the inputs that makes a scene a fair test of the decisions: every pair with n_c >= min_common has a D at least
    `least` (relative) away from max_dist — or it is an intended exact pair: exact = {(a, b): D}, input indices in either order, whose
    D must EQUAL the value given (scenes build those from dyadic numbers, so that no order of evaluation and no contraction rounds).
    -> the smallest margin over the other pairs."""
    md = float(max_dist)
    want = {tuple(sorted(k)): float(v) for k, v in (exact or {}).items()}
    seen, smallest = set(), INF
    for a, b, _ra, _rb, nc, D, _sim, _cons in rec["pairs"]:
        if nc < min_common or D != D:
            continue
        key = tuple(sorted((a, b)))
        if key in want:
            assert D == want[key], "pair %r was meant to give exactly %r: D = %r" % (key, want[key], D)
            seen.add(key)
            continue
        gap = INF if math.isinf(D) else abs(D - md) / max(md, TINY)
        assert gap >= least, "pair %r: D = %r is within %g (relative) of max_dist = %r" % (key, D, gap, md)
        smallest = min(smallest, gap)
    assert seen == set(want), "intended exact pairs that were not evaluated: %r" % (sorted(set(want) - seen),)
    return smallest

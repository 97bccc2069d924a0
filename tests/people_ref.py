"""NumPy / plain-loop restatement of stages B and C of dc_net_assemble_people (test helper, never on the product path).

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn has no consumer of `next_pred` and no part-candidate extraction (it stops at the
maps), so there is no reference output to hold the assembly to.  What is restated here is the definition in
include/deepcut_hip.h, on top of oracle/multiperson.py (the inverse of the label encoding of pose_data_layer.cpp:686-802): stage A
is `nms_candidates`, the predictions of stage B are `pairwise_positions`.  Small cases only."""
import math

import numpy as np

from oracle import multiperson as M

INF = float("inf")


def all_pairs_edges(num_joints=14):
    """Every ordered pair of joints, (a, c) with a != c, a-major: 182 edges for 14 joints — both directions of every pair."""
    return np.array([(a, c) for a in range(num_joints) for c in range(num_joints) if a != c], np.int32)


def one_direction_edges(num_joints=14):
    """As many edges as `all_pairs_edges`, but a -> c with a < c only: every pair is listed twice, so the second half is made of
    duplicates that the lowest-index rule must ignore."""
    half = [(a, c) for a in range(num_joints) for c in range(a + 1, num_joints)]
    return np.array(half + half, np.int32)


def edge_table(edges):
    """(a, c) -> the lowest edge index l with edges[l] == (a, c)."""
    lut = {}
    for l, (a, c) in enumerate(np.asarray(edges).reshape(-1, 2)):
        lut.setdefault((int(a), int(c)), l)
    return lut


def pair_costs_from_candidates(counts, dets, next_pred, edges, scale=1.0, mean=None, std=None):
    """counts [J], dets [J, MD, 5] (x, y, score, row, col) of ONE image, next_pred [2E, h, w] -> cost [J, J, MD, MD]."""
    J, MD = dets.shape[:2]
    lut = edge_table(edges)
    index, cells = {}, []
    for j in range(J):
        for i in range(int(counts[j])):
            index[j, i] = len(cells)
            cells.append((int(dets[j, i, 3]), int(dets[j, i, 4])))
    pred = M.pairwise_positions(next_pred, cells, scale, mean, std)  # [D, E, 2]
    cost = np.full((J, J, MD, MD), INF, np.float64)
    for a in range(J):
        for c in range(J):
            lf, lr = lut.get((a, c)), lut.get((c, a))
            if a == c or (lf is None and lr is None):
                continue
            for i in range(int(counts[a])):
                for k in range(int(counts[c])):
                    dist = []
                    if lf is not None:
                        d = pred[index[a, i], lf] - dets[c, k, :2]
                        dist.append(math.sqrt(d[0] * d[0] + d[1] * d[1]))
                    if lr is not None:
                        d = pred[index[c, k], lr] - dets[a, i, :2]
                        dist.append(math.sqrt(d[0] * d[0] + d[1] * d[1]))
                    cost[a, c, i, k] = scale * (sum(dist) / len(dist))
    return cost


def pair_costs(prob, loc, next_pred, edges, scale=1.0, threshold=0.1, radius=1, max_det=16, mean=None, std=None):
    """The maps of ONE image -> (counts [J], dets [J, MD, 5], cost [J, J, MD, MD]): stages A and B."""
    counts, dets = M.nms_candidates(prob, loc, scale, threshold, radius, max_det)
    return counts, dets, pair_costs_from_candidates(counts, dets, next_pred, edges, scale, mean, std)


def assemble(counts, dets, cost, max_cost, seed_threshold, max_people=32, min_joints=1, joint_order=None, gaps=None, stats=None):
    """Stage C on ONE image -> (people float64 [m, J, 3], cand int32 [m, J]).

    gaps (a dict, optional) receives how far the run was from deciding otherwise:
      "choice": the smallest difference, over all linking steps, between the chosen link and the best link that choosing it rules out
                (another link of the same person or of the same candidate that was still open);
      "max_cost": the smallest |L - max_cost| over every finite link cost that was compared with max_cost.
    A perturbation of the costs smaller than half of both cannot change the result: links that share neither the person nor the
    candidate with the chosen one stay open whichever of them goes first, so their order does not matter.

    stats (a dict, optional) receives what the run exercised:
      "tie_steps": the number of linking steps at which two or more open links had the minimal cost (the first in (p, i) order won);
      "max_links": the largest people x candidates of any joint, the length of the device's link list."""
    J = len(counts)
    order = list(range(J)) if joint_order is None else [int(j) for j in joint_order]
    seed = float(np.float32(seed_threshold))  # the C structure carries it as a float
    people = []
    g_choice, g_max = INF, INF
    tie_steps, max_links = 0, 0
    for j in order:
        m = int(counts[j])
        max_links = max(max_links, len(people) * m)
        used = [False] * m
        L = {}
        for p in range(len(people)):
            for i in range(m):
                s, n = 0.0, 0
                for a in range(J):
                    ia = people[p][a]
                    if a == j or ia < 0:
                        continue
                    v = float(cost[a, j, ia, i])
                    if math.isfinite(v):
                        s += v
                        n += 1
                L[p, i] = s / n if n else INF
                if n:
                    g_max = min(g_max, abs(L[p, i] - max_cost))
        while True:
            best = None
            for p in range(len(people)):
                for i in range(m):
                    if used[i] or people[p][j] >= 0:
                        continue
                    if L[p, i] <= max_cost and (best is None or L[p, i] < best[0]):  # p, then i ascending: the first of equals stays
                        best = (L[p, i], p, i)
            if best is None:
                break
            _, bp, bi = best
            if stats is not None:
                tie_steps += sum(1 for p in range(len(people)) if people[p][j] < 0
                                 for i in range(m) if not used[i] and L[p, i] == best[0]) >= 2
            if gaps is not None:
                for p in range(len(people)):
                    for i in range(m):
                        if (p, i) != (bp, bi) and (p == bp or i == bi) and not used[i] and people[p][j] < 0:
                            g_choice = min(g_choice, L[p, i] - best[0])
            people[bp][j] = bi
            used[bi] = True
        for i in range(m):
            if not used[i] and float(dets[j, i, 2]) >= seed and len(people) < max_people:
                people.append([-1] * J)
                people[-1][j] = i
    kept = [p for p in people if sum(1 for c in p if c >= 0) >= min_joints]
    out = np.zeros((len(kept), J, 3), np.float64)
    cand = np.full((len(kept), J), -1, np.int32)
    for q, p in enumerate(kept):
        for a in range(J):
            if p[a] >= 0:
                cand[q, a] = p[a]
                out[q, a] = dets[a, p[a], :3]
    if gaps is not None:
        gaps["choice"], gaps["max_cost"] = g_choice, g_max
    if stats is not None:
        stats["tie_steps"], stats["max_links"] = tie_steps, max_links
    return out, cand


# ---- planted scenes (tests/test_gpu_people.py) ---------------------------------------------------------------------------------
def round_to_bf16(x):
    """float values -> the nearest bfloat16 values (round to nearest even), as float32: numbers float16 and bfloat16 both hold exactly
    at the magnitudes used here (|x| in [2^-14, 65504] or 0)."""
    a = np.ascontiguousarray(x, np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    out = u.astype(np.uint32).view(np.float32).reshape(a.shape)
    return np.where(np.abs(out) < 2.0 ** -14, np.float32(0), out)


def planted_scene(h, w, edges, mean, std, scale=1.0, num_joints=14, sixteen_bit=False):
    """Maps [J, h, w], [2J, h, w], [2E, h, w] (float32) with three planted people of `num_joints` joints each and two stray peaks.
    Person q's joint j sits near x = 40 + 90 q, y = 16 + 12.5 j (network pixels / scale), on a cell of its own; its score peak is the
    only non-zero value around, `loc_pred` refines the cell to the planted point and `next_pred` at that cell, written with
    oracle.multiperson.encode_targets, points at the same person's other joints on every edge that leaves j.  The strays (joints 3
    and 9) are peaks whose `next_pred` is zero: they point at their own cell (+ mean), far from everybody.
    sixteen_bit: every value is rounded to one that float16 and bfloat16 hold exactly (the predictions are then off by up to half a
    pixel or so: far below the 90 px between people).
    -> (prob, loc, next, joints [3, J, 2] planted points in image pixels, strays [(joint, x, y)])."""
    edges = np.asarray(edges).reshape(-1, 2)
    E = edges.shape[0]
    mean = np.zeros((E, 2)) if mean is None else np.asarray(mean, np.float64).reshape(E, 2)
    std = np.ones((E, 2)) if std is None else np.asarray(std, np.float64).reshape(E, 2)
    rs = np.random.RandomState(7)
    prob = np.zeros((num_joints, h, w), np.float32)
    loc = np.zeros((2 * num_joints, h, w), np.float32)
    nxt = np.zeros((2 * E, h, w), np.float32)
    q16 = round_to_bf16 if sixteen_bit else (lambda v: np.asarray(v, np.float32))
    joints = np.zeros((3, num_joints, 2), np.float64)
    cells = {}
    for q in range(3):
        for j in range(num_joints):
            x = (40.0 + 90.0 * q + rs.uniform(-6, 6)) / scale
            y = (16.0 + 12.5 * j + rs.uniform(-2, 2)) / scale
            r, c = int(y * scale // M.STRIDE), int(x * scale // M.STRIDE)
            assert 0 <= r < h and 0 <= c < w
            # the refinement is what the map can hold: the planted point is what the (rounded) value decodes to
            lt, _ = M.encode_targets((x, y), (x, y), (r, c), scale, (0, 0), (1, 1))
            lt = q16(lt).astype(np.float64)
            pt = np.array([c * M.STRIDE + 0.5 * M.STRIDE, r * M.STRIDE + 0.5 * M.STRIDE])
            joints[q, j] = (pt + lt * M.LOCREF) / scale
            cells[q, j] = (r, c)
            loc[2 * j, r, c], loc[2 * j + 1, r, c] = lt
            prob[j, r, c] = (0.875, 0.75, 0.625)[q]
    for q in range(3):
        for l, (a, c) in enumerate(edges):
            _, nt = M.encode_targets(joints[q, a], joints[q, c], cells[q, int(a)], scale, mean[l], std[l])
            r, col = cells[q, int(a)]
            nxt[2 * l, r, col], nxt[2 * l + 1, r, col] = q16(nt)
    strays = []
    for j, (x, y) in ((3, (85.0, 186.0)), (9, (176.0, 22.0))):
        r, c = int(y // M.STRIDE), int(x // M.STRIDE)
        assert prob[j, max(0, r - 1):r + 2, max(0, c - 1):c + 2].max() == 0
        prob[j, r, c] = 0.5625
        strays.append((j, (c * M.STRIDE + 4.0) / scale, (r * M.STRIDE + 4.0) / scale))
    return prob, loc, nxt, joints, strays


def crowded_scene(h, w, edges, seed, peaks=40, lattice=False, sixteen_bit=False, num_joints=14):
    """Maps [J, h, w], [2J, h, w], [2E, h, w] (float32) with `peaks` isolated score peaks per joint, on cells with even row and column
    (two peaks are at least 2 cells apart: each is alone in its 3x3 neighbourhood, a candidate at radius 1).  Scores lie in
    [0.6, 0.95]: drawn and rounded to float32, or — sixteen_bit — distinct values that float16 and bfloat16 both hold exactly, so that
    the candidate order does not hang on a tie.  `loc_pred` is small and random and `next_pred` standard normal (the caller's mean /
    std spread the predictions over the image), both rounded with round_to_bf16 when sixteen_bit.
    lattice: `loc_pred` = `next_pred` = 0.  Without mean / std at scale 1 every candidate sits on its cell centre and predicts that
    centre for every edge, so every pair cost is the distance between two points of a 16-pixel lattice: equal costs are exactly equal
    in double, on the device and here."""
    E = np.asarray(edges).reshape(-1, 2).shape[0]
    rs = np.random.RandomState(seed)
    spots = [(r, c) for r in range(0, h, 2) for c in range(0, w, 2)]
    assert len(spots) >= peaks
    prob = np.zeros((num_joints, h, w), np.float32)
    grid16 = np.arange(154, 244) / 256.0  # the 8-bit-mantissa values of [0.6, 0.95]: exact in both 16-bit types
    for j in range(num_joints):
        where = rs.choice(len(spots), peaks, replace=False)
        score = rs.choice(grid16, peaks, replace=False) if sixteen_bit else rs.uniform(0.6, 0.95, peaks)
        for s, v in zip(where, score):
            prob[j][spots[s]] = np.float32(v)
    if lattice:
        return prob, np.zeros((2 * num_joints, h, w), np.float32), np.zeros((2 * E, h, w), np.float32)
    q16 = round_to_bf16 if sixteen_bit else (lambda v: np.asarray(v, np.float32))
    loc = q16(rs.uniform(-0.3, 0.3, (2 * num_joints, h, w)))
    nxt = q16(rs.randn(2 * E, h, w))
    return prob, loc, nxt

"""Crafted scenes for stage E of the people assembly (dedupe): host arrays for dc_dedupe_people together with the survivors derived by
hand.  tests/test_dedupe_host.py holds the float64 restatement (tests/dedupe_ref.py) to them and checks that every decision is far
from max_dist; tests/test_gpu_dedupe.py holds the device to the restatement.  Every coordinate and score is dyadic unless said
otherwise, so the arithmetic of the intended ties is exact in any order of evaluation.

A scene is a dict: "people" [nb, P, J, 3], "n" [nb], "cand" [nb, P, J] or None, "params" (max_dist, min_common, min_size, sigma,
absorb), "kept": per image the input indices that survive, "by": per image {suppressed input index: its killer}, "exact": per image
{(a, b): D} for the pairs whose D is meant to be exactly that value (a tie with max_dist, or one ulp away from it), and optionally
"people_out" / "cand_out": per image the expected arrays where copying alone does not give them (absorb)."""
import numpy as np

NAN, INF = float("nan"), float("inf")


def _scene(people, n, params, kept, by, cand=None, exact=None, **more):
    people = np.ascontiguousarray(people, np.float64)
    nb = people.shape[0]
    p = dict(max_dist=0.5, min_common=1, min_size=16.0, sigma=None, absorb=False)
    p.update(params)
    sc = dict(people=people, n=np.asarray(n, np.int32), cand=None if cand is None else np.ascontiguousarray(cand, np.int32), params=p,
              kept=[list(k) for k in kept], by=[dict(b) for b in by], exact=[dict(e) for e in (exact or [{}] * nb)])
    sc.update(more)
    return sc


def skeleton(J):
    """J joints, 8 px apart in x and alternating 0 / 40 in y: the x extent 8 (J - 1) is the size for J >= 6 (min_size 32)."""
    return np.array([[8.0 * j, 40.0 * (j % 2)] for j in range(J)])


def chain():
    """(a) J = 1, people at x = 0, 8, 16 with descending scores, min_size 16: D = 64 / 256 = 0.25 between neighbours, 1.0 between the
    ends.  The second is suppressed by the first and therefore does not suppress the third."""
    ppl = np.zeros((1, 3, 1, 3))
    ppl[0, :, 0, 0] = [0.0, 8.0, 16.0]
    ppl[0, :, 0, 2] = [0.875, 0.75, 0.625]
    return _scene(ppl, [3], dict(max_dist=0.5), kept=[[0, 2]], by=[{1: 0}], exact=[{(0, 1): 0.25, (1, 2): 0.25, (0, 2): 1.0}])


def exact_tie(above):
    """(b) J = 4, A holds the corners of a 16 px square (s = 16), B the same corners moved by 8 px in one coordinate each and holds the
    first 1, 2 or 4 of them (images 0, 1, 2): every term is 64 / 256, so D = 0.25 exactly for n_c = 1, 2, 4.  max_dist = 0.25: a tie,
    suppressed.  above: max_dist is the double just below 0.25, D is one ulp above it, kept."""
    A = np.array([[0.0, 0.0], [16.0, 0.0], [0.0, 16.0], [16.0, 16.0]])
    move = np.array([[8.0, 0.0], [0.0, 8.0], [-8.0, 0.0], [0.0, -8.0]])
    ppl = np.zeros((3, 2, 4, 3))
    for b, nc in enumerate((1, 2, 4)):
        ppl[b, 0, :, :2], ppl[b, 0, :, 2] = A, 0.875
        ppl[b, 1, :, :2] = A + move
        ppl[b, 1, :nc, 2] = 0.5
    md = float(np.nextafter(0.25, 0.0)) if above else 0.25
    kept = [[0, 1]] * 3 if above else [[0]] * 3
    by = [{}] * 3 if above else [{1: 0}] * 3
    return _scene(ppl, [2, 2, 2], dict(max_dist=md), kept=kept, by=by, exact=[{(0, 1): 0.25}] * 3)


def equal_scores():
    """(c) Three people of one score: 0 far away, 1 and 2 four pixels apart (D = 16 / 256).  The lower index ranks first: 1 suppresses 2."""
    ppl = np.zeros((1, 3, 1, 3))
    ppl[0, :, 0, 0] = [512.0, 0.0, 4.0]
    ppl[0, :, 0, 2] = 0.5
    return _scene(ppl, [3], dict(max_dist=0.5), kept=[[0, 1]], by=[{2: 1}])


def _crowd(J, perm_seed):
    """256 people, rank r at its own place on a 16 x 16 grid of 1024 px, every joint score 1 - r / 512 (so S descends with r, exactly),
    input index = a fixed permutation of the rank.  -> (pose [256, J, 3] BY RANK, perm: rank -> input index)."""
    sk = skeleton(J)
    pose = np.zeros((256, J, 3))
    for r in range(256):
        pose[r, :, 0] = sk[:, 0] + 1024.0 * (r % 16)
        pose[r, :, 1] = sk[:, 1] + 1024.0 * (r // 16)
        pose[r, :, 2] = 1.0 - r / 512.0
    perm = np.random.RandomState(perm_seed).permutation(256) if perm_seed is not None else np.arange(256)
    return pose, perm


def _by_input(pose, perm):
    ppl = np.zeros((1, 256) + pose.shape[1:])
    ppl[0, perm] = pose
    return ppl


def crowd_nobody(J=14, perm_seed=5):
    """(d) n = P = 256, nobody similar (D >= 1024^2 / 104^2): the output equals the input."""
    pose, perm = _crowd(J, perm_seed)
    return _scene(_by_input(pose, perm), [256], dict(max_dist=0.5, min_common=3, min_size=32.0), kept=[range(256)], by=[{}])


def crowd_everybody(J=14, perm_seed=5):
    """(d) everybody within a pixel of the best-scored person (rank r moved by r / 256 px in x): one survivor."""
    pose, perm = _crowd(J, perm_seed)
    sk = skeleton(J)
    for r in range(256):
        pose[r, :, 0], pose[r, :, 1] = sk[:, 0] + r / 256.0, sk[:, 1]
    return _scene(_by_input(pose, perm), [256], dict(max_dist=0.5, min_common=3, min_size=32.0), kept=[[int(perm[0])]],
                  by=[{int(perm[r]): int(perm[0]) for r in range(1, 256)}])


# (rank of the victim, rank of its killer): pairs that straddle the words of the mask, 63|64, 127|128 and 191|192, and killers that are
# the last-ranked kept person of another word than the victim's (127 -> 200, 191 -> 255)
CROWD_VICTIMS = ((64, 63), (128, 127), (192, 191), (200, 127), (255, 191))


def crowd_words(J=14, perm_seed=5):
    """(d) the victims of CROWD_VICTIMS stand d = 5 s / 8 right of their killers, s = 8 (J - 1) being everybody's size: D = 25 / 64, below
    0.5.  Rank 65 stands d right of rank 64 and 2 d from rank 63 (D = 100 / 64): its only similar better-ranked person is suppressed,
    so it survives."""
    pose, perm = _crowd(J, perm_seed)
    d = 5.0 * (J - 1)
    for v, k in CROWD_VICTIMS:
        pose[v, :, :2] = pose[k, :, :2] + [d, 0.0]
    pose[65, :, :2] = pose[64, :, :2] + [d, 0.0]
    victims = {v for v, _ in CROWD_VICTIMS}
    return _scene(_by_input(pose, perm), [256], dict(max_dist=0.5, min_common=3, min_size=32.0),
                  kept=[sorted(int(perm[r]) for r in range(256) if r not in victims)],
                  by=[{int(perm[v]): int(perm[k]) for v, k in CROWD_VICTIMS}])


def batch_edges():
    """(e) J = 32 with a sigma per joint, nb = 3 with n = 8, 0 and 1 in one call.  Image 0: four pairs of people, the second of each
    pair 16 px right of the first; sigma_j = 1 or 2 alternating, s = 248: D = (256 / 248^2) (1 + 1/4) / 2, far below 0.5."""
    J = 32
    sk = skeleton(J)
    ppl = np.zeros((3, 8, J, 3))
    for q in range(8):
        ppl[0, q, :, 0] = sk[:, 0] + 2048.0 * (q // 2) + 16.0 * (q % 2)
        ppl[0, q, :, 1] = sk[:, 1]
        ppl[0, q, :, 2] = 0.5 + (q % 2) * 0.25 - q / 64.0  # the second of a pair is the better one
    ppl[2, 0, :, :2], ppl[2, 0, :, 2] = sk, 0.5
    sigma = [1.0 + (j % 2) for j in range(J)]
    return _scene(ppl, [8, 0, 1], dict(max_dist=0.5, min_common=32, min_size=32.0, sigma=sigma), kept=[[1, 3, 5, 7], [], [0]],
                  by=[{0: 1, 2: 3, 4: 5, 6: 7}, {}, {}])


def one_joint_one_person():
    """(e) J = 1, P = 1: one person, then nobody."""
    ppl = np.zeros((2, 1, 1, 3))
    ppl[0, 0, 0] = [3.0, 5.0, 0.5]
    return _scene(ppl, [1, 0], dict(max_dist=0.5), kept=[[0], []], by=[{}, {}])


def special_values():
    """(f) J = 3, min_common 2, min_size 32.  0: the model person.  1: the same place, but holds joint 0 only: n_c = 1, never similar.
    2: the same place with a NaN x on a held joint: every D with it is a NaN, no suppression either way.  3 / 4: joints 0 and 1 of the
    model and a far joint 2 whose score is a NaN / negative: not held, so n_c = 2 and D = 0 — suppressed by 0.  5: an infinite score on
    one joint, far away: ranks first although 6, beside it, has the larger finite scores — 5 suppresses 6, not the reverse."""
    base = np.array([[0.0, 0.0], [8.0, 0.0], [0.0, 8.0]])
    ppl = np.zeros((1, 7, 3, 3))
    ppl[0, :, :, :2] = base
    ppl[0, 0, :, 2] = 0.875
    ppl[0, 1, 0, 2] = 0.5
    ppl[0, 2, :, 2] = 0.75
    ppl[0, 2, 1, 0] = NAN
    for q, bad in ((3, NAN), (4, -1.0)):
        ppl[0, q, :2, 2] = 0.625
        ppl[0, q, 2] = [4096.0, 4096.0, bad]
    ppl[0, 5, :, :2] = base + [2048.0, 0.0]
    ppl[0, 5, :, 2] = [INF, 0.125, 0.125]
    ppl[0, 6, :, :2] = base + [2052.0, 0.0]
    ppl[0, 6, :, 2] = 0.9375
    return _scene(ppl, [7], dict(max_dist=0.5, min_common=2, min_size=32.0), kept=[[0, 1, 2, 5]], by=[{3: 0, 4: 0, 6: 5}])


def fragments(absorb, with_cand=True):
    """(g) J = 14.  A (index 0) holds 0..6 from stage C and 7..13 as fills (cand -2) at the skeleton; B (index 2) the reverse, its own
    7..12 93 px below A's fills and no joint 13: D(A, B) = (7 * 5 + 6 * 93^2) / (13 s^2) = 0.369 with s = 104.  C (index 1, scored
    below B) is B two pixels further, and holds joint 13 from stage C where B has nothing: D(A, C) = 0.401.  T (index 3) holds 7..12
    only, exactly where B does: D(A, T) = 93^2 / 104^2 = 0.7997 > 0.5 on the input, and 0 had the absorbed joints counted.  absorb: A survives with 0..6 its own,
    7..12 B's (the first-ranked donor, although C has the lower index) and 13 C's; T survives either way."""
    J, sk = 14, skeleton(14)
    ppl = np.zeros((1, 4, J, 3))
    cand = np.full((1, 4, J), -1, np.int32)
    A, C_, B, T = 0, 1, 2, 3
    ppl[0, A, :, :2] = sk
    ppl[0, A, :7, 2], cand[0, A, :7] = 0.875, 3 + np.arange(7)
    ppl[0, A, 7:, 2], cand[0, A, 7:] = 0.25, -2
    for q, off, sc, c0 in ((B, 0.0, 0.75, 20), (C_, 2.0, 0.625, 40)):
        ppl[0, q, :7, :2] = sk[:7] + [2.0 + off, 1.0]
        ppl[0, q, :7, 2], cand[0, q, :7] = 0.25, -2
        ppl[0, q, 7:, :2] = sk[7:] + [off, 93.0]
        ppl[0, q, 7:, 2], cand[0, q, 7:] = sc, c0 + np.arange(7)
    ppl[0, B, 13], cand[0, B, 13] = 0.0, -1
    ppl[0, T, 7:, :2] = sk[7:] + [0.0, 93.0]
    ppl[0, T, 7:, 2], cand[0, T, 7:] = 0.5, 50 + np.arange(7)
    ppl[0, T, 13, 2], cand[0, T, 13] = 0.0, -1  # (B's joint 13 is missing, so T leaves it out as well)
    exp_p, exp_c = ppl[0, [A, T]].copy(), cand[0, [A, T]].copy()
    if absorb:
        exp_p[0, 7:13], exp_c[0, 7:13] = ppl[0, B, 7:13], cand[0, B, 7:13]
        exp_p[0, 13], exp_c[0, 13] = ppl[0, C_, 13], cand[0, C_, 13]
    return _scene(ppl, [4], dict(max_dist=0.5, min_common=3, min_size=32.0, absorb=absorb), kept=[[A, T]], by=[{B: A, C_: A}], cand=cand,
                  people_out=[exp_p], cand_out=[exp_c])


def absorb_without_cand():
    """(g) cand = NULL: assigned == held.  J = 4: A holds 0..2, B (beside it) holds 1..3: A absorbs joint 3 and keeps its own 1 and 2."""
    ppl = np.zeros((1, 2, 4, 3))
    sq = np.array([[0.0, 0.0], [16.0, 0.0], [0.0, 16.0], [16.0, 16.0]])
    ppl[0, 0, :3, :2], ppl[0, 0, :3, 2] = sq[:3], 0.875
    ppl[0, 1, 1:, :2], ppl[0, 1, 1:, 2] = sq[1:] + [1.0, 0.0], 0.5
    exp_p = ppl[0, [0]].copy()
    exp_p[0, 3] = ppl[0, 1, 3]
    return _scene(ppl, [2], dict(max_dist=0.5, min_common=2, min_size=16.0, absorb=True), kept=[[0]], by=[{1: 0}],
                  people_out=[exp_p], cand_out=[np.array([[0, 0, 0, 0]], np.int32)])


SCENES = {
    "a_chain": chain,
    "b_tie": lambda: exact_tie(False),
    "b_one_ulp_above": lambda: exact_tie(True),
    "c_equal_scores": equal_scores,
    "d_nobody": crowd_nobody,
    "d_everybody": crowd_everybody,
    "d_words": crowd_words,
    "d_words_in_rank_order": lambda: crowd_words(perm_seed=None),
    "e_batch_j32": batch_edges,
    "e_j1_p1": one_joint_one_person,
    "e_j32_p256": lambda: crowd_words(J=32),
    "f_special": special_values,
    "g_absorb": lambda: fragments(True),
    "g_no_absorb": lambda: fragments(False),
    "g_absorb_no_cand": absorb_without_cand,
}
_made = {}


def scene(name):
    """The scene and, once for every test that needs it, the restatement's result on it (made by the caller through `reference`)."""
    if name not in _made:
        _made[name] = SCENES[name]()
    return _made[name]


_refs = {}


def reference(name):
    """dedupe_ref_batch on the scene, computed once and shared: (n_out, people, cand, kept_from, suppressed_by, records)."""
    import dedupe_ref as E

    if name not in _refs:
        sc = scene(name)
        _refs[name] = E.dedupe_ref_batch(sc["people"], sc["n"], sc["cand"], **sc["params"])
    return _refs[name]

"""Float64 NumPy restatement of the multi-scale fusion rule of dc_group_fuse_maps (test helper, never on the product path), and a
planted pyramid to run the fused maps through the people assembly.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and combines nothing across scales, so there is no
reference output to hold the fusion to.  What is restated here is the definition in include/deepcut_hip.h; the only thing of the
reference's in it is the label encoding of pose_data_layer.cpp:686-802 (oracle/multiperson.py), which the gain / bias of `loc_pred`
and `next_pred` follow.

The device sums in float32; `fuse` returns, beside the fused maps, A = the same sums taken over the absolute values of every product
and of the bias.  The rule has about ten roundings per member (two weights, four corner products, three sums, the outer products, gain
and bias, the running sum, the final 1/M), each relative to a term of A, so |device - restatement| <= BOUND * A element by element."""
import numpy as np

import people_ref as R
from oracle import multiperson as M

BOUND = 16 * 2.0 ** -24
NAMES = ("prob", "loc_pred", "next_pred")


def sample_axis(n_base, n_member, q):
    """Base cells 0..n_base-1 of one axis -> (i0, i1, f): the two member cells and the float32 weight of the second."""
    u = ((8.0 * np.arange(n_base, dtype=np.float64) + 4.0) * q - 4.0) / 8.0
    u = np.minimum(np.maximum(u, 0.0), float(n_member - 1))
    i0 = np.floor(u).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_member - 1)
    return i0, i1, (u - i0).astype(np.float32).astype(np.float64)


def gain_bias(k, channels, rho, mean, std):
    """Map k (0 prob, 1 loc_pred, 2 next_pred) -> (gain [C], bias [C]): computed in double, carried as float32."""
    gain = np.full(channels, 1.0 if k == 0 else rho, np.float64)
    bias = np.zeros(channels, np.float64)
    if k == 2:
        mu = np.zeros(channels) if mean is None else np.asarray(mean, np.float64).reshape(-1)
        sd = np.ones(channels) if std is None else np.asarray(std, np.float64).reshape(-1)
        bias = (rho - 1.0) * mu / sd
    return gain.astype(np.float32).astype(np.float64), bias.astype(np.float32).astype(np.float64)


def fuse(maps_per_member, scales, base, mean=None, std=None):
    """maps_per_member: per member a (prob, loc_pred, next_pred) triple of [NB, C, H_m, W_m] arrays (any entry None for every member:
    that map takes no part).  -> (fused, A): two triples of float64 [NB, C, H_b, W_b] arrays (None where the map took no part)."""
    nm = len(maps_per_member)
    s_b = float(scales[base])
    inv_m = float(np.float32(1.0) / np.float32(nm))
    fused, bound = [], []
    for k in range(3):
        if maps_per_member[0][k] is None:
            fused.append(None), bound.append(None)
            continue
        hb, wb = maps_per_member[base][k].shape[2:]
        acc = a_acc = 0.0
        for m in range(nm):
            a = np.asarray(maps_per_member[m][k], np.float64)
            q = 1.0 if m == base else float(scales[m]) / s_b
            rho = 1.0 if m == base else s_b / float(scales[m])
            y0, y1, fy = sample_axis(hb, a.shape[2], q)
            x0, x1, fx = sample_axis(wb, a.shape[3], q)
            fy, fx = fy[:, None], fx[None, :]
            a00, a01 = a[:, :, y0][:, :, :, x0], a[:, :, y0][:, :, :, x1]
            a10, a11 = a[:, :, y1][:, :, :, x0], a[:, :, y1][:, :, :, x1]
            val = (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11)
            mag = (1 - fy) * ((1 - fx) * np.abs(a00) + fx * np.abs(a01)) + fy * ((1 - fx) * np.abs(a10) + fx * np.abs(a11))
            gain, bias = gain_bias(k, a.shape[1], rho, mean, std)
            acc = acc + (val * gain[None, :, None, None] + bias[None, :, None, None])
            a_acc = a_acc + (mag * np.abs(gain)[None, :, None, None] + np.abs(bias)[None, :, None, None])
        fused.append(acc * inv_m), bound.append(a_acc * inv_m)
    return tuple(fused), tuple(bound)


def worst_ratio(got, ref, a):
    """max over the elements of |got - ref| / (BOUND * A); an element with A = 0 must match exactly."""
    err = np.abs(np.asarray(got, np.float64) - ref)
    lim = BOUND * a
    if (err[lim == 0] != 0).any():
        return float("inf")
    return float((err[lim > 0] / lim[lim > 0]).max()) if (lim > 0).any() else 0.0


# ---- a planted pyramid ---------------------------------------------------------------------------------------------------------------
PEAKS = (0.9, 0.85, 0.8)  # person q's score peak: distinct, so the candidate order does not hang on a rounding
THRESHOLD = 0.45
RADIUS_NET = 12.0        # support of the score bump around a joint, in network pixels of the base member


def planted_pyramid(shapes, scales, base, edges, mean, std, num_joints=14, sixteen_bit=False):
    """Three people of `num_joints` joints, given in image pixels, rendered into every member's maps at its own scale.
    shapes: per member the (h, w) of its maps.  Person q's joint j lies within 1.5 network pixels of the centre of base cell
    (2 + j, 5 + 11 q).  `prob` is the same smooth bump of the image-space distance d between a cell's point and the joint at every
    scale, peak * (1 - (d / R)^2)^2 inside R = RADIUS_NET / s_b; `loc_pred` and `next_pred` hold the correctly encoded values
    (oracle.multiperson.encode_targets at the member's scale) on every cell within R + 2 cells of the joint, which covers all four
    corners of every sample that touches the bump: the fields are linear in the cell position there, so their fusion is exact.
    sixteen_bit: every value rounded to one float16 and bfloat16 both hold (people_ref.round_to_bf16).
    Asserted on the restatement alone: every planted joint is a strict 3x3 maximum of the fused `prob` by at least 1e-3, and no other
    cell reaches THRESHOLD.
    -> dict: maps (per member a triple of [1, C, h, w] float32), fused / A (the restatement's), truth [3, J, 2] (the planted joints),
    joints [3, J, 2] (what the fused loc_pred of the restatement decodes to at the joint's cell), cells [3][J] (row, col) on the base grid."""
    edges = np.asarray(edges).reshape(-1, 2)
    ne = edges.shape[0]
    mean = np.zeros((ne, 2)) if mean is None else np.asarray(mean, np.float64).reshape(ne, 2)
    std = np.ones((ne, 2)) if std is None else np.asarray(std, np.float64).reshape(ne, 2)
    s_b = float(scales[base])
    hb, wb = shapes[base]
    rs = np.random.RandomState(11)
    truth = np.zeros((3, num_joints, 2))
    cells = [[None] * num_joints for _ in range(3)]
    for q in range(3):
        for j in range(num_joints):
            r, c = 2 + j, 5 + 11 * q
            assert r < hb - 2 and c < wb - 2, "the base grid %dx%d is too small for the planted people" % (hb, wb)
            truth[q, j] = (np.array([c * M.STRIDE + 4.0, r * M.STRIDE + 4.0]) + rs.uniform(-1.5, 1.5, 2)) / s_b
            cells[q][j] = (r, c)
    q16 = R.round_to_bf16 if sixteen_bit else (lambda v: np.asarray(v, np.float32))
    out_edges = [[l for l in range(ne) if edges[l, 0] == j] for j in range(num_joints)]
    maps = []
    for (h, w), s in zip(shapes, scales):
        s = float(s)
        prob = np.zeros((num_joints, h, w), np.float32)
        loc = np.zeros((2 * num_joints, h, w), np.float32)
        nxt = np.zeros((2 * ne, h, w), np.float32)
        px = (np.arange(w) * M.STRIDE + 4.0) / s
        py = (np.arange(h) * M.STRIDE + 4.0) / s
        radius, reach = RADIUS_NET / s_b, RADIUS_NET / s_b + 2 * M.STRIDE / s
        owner = np.full((num_joints, h, w), -1)
        for q in range(3):
            for j in range(num_joints):
                x, y = truth[q, j]
                d2 = (py[:, None] - y) ** 2 + (px[None, :] - x) ** 2
                prob[j] += (PEAKS[q] * np.maximum(0.0, 1.0 - d2 / radius ** 2) ** 2).astype(np.float32)
                for r in np.nonzero(np.abs(py - y) <= reach)[0]:
                    for c in np.nonzero(np.abs(px - x) <= reach)[0]:
                        assert owner[j, r, c] < 0, "two people's neighbourhoods of joint %d overlap" % j
                        owner[j, r, c] = q
                        lt, _ = M.encode_targets(truth[q, j], truth[q, j], (r, c), s, (0, 0), (1, 1))
                        loc[2 * j:2 * j + 2, r, c] = lt
                        for l in out_edges[j]:
                            _, nt = M.encode_targets(truth[q, j], truth[q, edges[l, 1]], (r, c), s, mean[l], std[l])
                            nxt[2 * l:2 * l + 2, r, c] = nt
        maps.append(tuple(q16(a)[None] for a in (prob, loc, nxt)))
    fused, bound = fuse(maps, scales, base, mean, std)
    # the restatement alone: the planted joints are the candidates, decided with room to spare
    fp = fused[0][0]
    planted = np.zeros(fp.shape, bool)
    joints = np.zeros_like(truth)
    for q in range(3):
        for j in range(num_joints):
            r, c = cells[q][j]
            planted[j, r, c] = True
            window = fp[j, r - 1:r + 2, c - 1:c + 2].copy()
            window[1, 1] = -np.inf
            assert fp[j, r, c] - window.max() >= 1e-3, "joint (%d, %d) is not a strict 3x3 maximum by 1e-3" % (q, j)
            assert fp[j, r, c] >= THRESHOLD + 1e-3
            lx, ly = fused[1][0][2 * j:2 * j + 2, r, c]
            joints[q, j] = (c * M.STRIDE + 4.0 + lx * M.LOCREF) / s_b, (r * M.STRIDE + 4.0 + ly * M.LOCREF) / s_b
    assert (fp[~planted] < THRESHOLD - 1e-3).all(), "a cell that is no planted joint reaches the threshold"
    assert np.abs(joints - truth).max() <= (1.0 if sixteen_bit else 1e-4), np.abs(joints - truth).max()
    return dict(maps=maps, fused=fused, A=bound, truth=truth, joints=joints, cells=cells)


def assemble_fused(fused, edges, scale, mean, std, threshold=THRESHOLD, radius=1, max_det=8, max_cost=20.0, seed_threshold=0.5,
                   min_joints=2, gaps=None):
    """The fused maps of ONE image ([C, h, w] each) through people_ref: -> (counts, dets, cost, people, cand)."""
    counts, dets, cost = R.pair_costs(fused[0], fused[1], fused[2], edges, scale, threshold, radius, max_det, mean, std)
    people, cand = R.assemble(counts, dets, cost, max_cost, seed_threshold, 32, min_joints, gaps=gaps)
    return counts, dets, cost, people, cand



# ---- what tests/test_fuse_host.py and tests/test_gpu_fuse.py share ---------------------------------------------------------------------
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))  # the statistics tests/test_gpu_people.py uses
SCALES = (0.7, 1.0, 1.3)
_scene = {}


def planted(sixteen_bit):
    """The planted pyramid of a 200 x 264 image at SCALES, base = the middle scale: computed once per process, never written to."""
    if sixteen_bit not in _scene:
        import caffe

        shapes = [tuple(v // 8 for v in caffe.canvas_size(200, 264, s)) for s in SCALES]
        _scene[sixteen_bit] = planted_pyramid(shapes, SCALES, 1, R.all_pairs_edges(), MEAN, STD, sixteen_bit=sixteen_bit)
    return _scene[sixteen_bit]


def match_people(people, joints):
    """The planted person every returned person is, by the first joint -> a permutation of 0..2."""
    return [int(np.argmin(np.abs(joints[:, 0, 0] - p[0, 0]))) for p in people]

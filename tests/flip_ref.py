"""Float64 NumPy restatement of the mirrored fusion rule of dc_group_fuse_maps_mirrored (test helper, never on the product path), and a
planted pyramid with mirrored members to run the fused maps through the people assembly.  In the manner of tests/fuse_ref.py, whose
`sample_axis`, `worst_ratio`, `BOUND`, `MEAN` and `STD` it reuses.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and mirrors nothing on the pose path, so there is no
reference output to hold the rule to.  What is restated here is the definition in include/deepcut_hip.h.

The bound: a mirrored member costs the device exactly the roundings an unmirrored one does — the gain is still one float, each weight
still one float, the same products and sums — so |device - restatement| <= BOUND * A = 16 * 2^-24 * A element by element, as in
fuse_ref.  A base cell whose u falls within an ulp of an integer may floor differently on the device; the bilinear value is
continuous there (weight 1 on one cell against weight 0 on its neighbour), so it stays inside the bound and is not special-cased."""
import numpy as np

import people_ref as R
from fuse_ref import BOUND, MEAN, PEAKS, RADIUS_NET, STD, THRESHOLD, sample_axis, worst_ratio  # noqa: F401  (shared with the tests)
from oracle import multiperson as M

MIRROR_MPII14 = (5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13)  # restated, not imported: pose.MIRROR_MPII14 is checked against it


def sample_axis_mirrored(n_base, n_member, q, ws):
    """The x axis of a mirrored member: base columns 0..n_base-1 -> (i0, i1, f).  ws = (image width - 1) * the member's scale."""
    u = ((ws - (8.0 * np.arange(n_base, dtype=np.float64) + 4.0) * q) - 4.0) / 8.0
    u = np.minimum(np.maximum(u, 0.0), float(n_member - 1))
    i0 = np.floor(u).astype(np.int64)
    i1 = np.minimum(i0 + 1, n_member - 1)
    return i0, i1, (u - i0).astype(np.float32).astype(np.float64)


def mirrored_edges(edges, pi):
    """edges [E, 2], pi [J] -> [E]: for edge l = (a, c) the lowest-index edge equal to (pi[a], pi[c])."""
    edges = np.asarray(edges).reshape(-1, 2)
    first = {}
    for l, (a, c) in enumerate(edges):
        first.setdefault((int(a), int(c)), l)
    return np.array([first[(int(pi[a]), int(pi[c]))] for a, c in edges], np.int64)


def mirror_gain_bias(k, channels, rho, pi, lprime, mean, std, sign=-1.0):
    """Map k of a MIRRORED member -> (gain [C], bias [C], source channel [C]): gain and bias computed in double, carried as float32.
    sign = -1 is the rule (the x components change sign); sign = +1 with pi and lprime the identity is the unmirrored rule."""
    ch = np.arange(channels)
    if k == 0:
        return np.ones(channels), np.zeros(channels), np.asarray(pi)[ch]
    if k == 1:
        gain = np.where(ch % 2 == 0, sign * rho, rho).astype(np.float64)
        return gain.astype(np.float32).astype(np.float64), np.zeros(channels), 2 * np.asarray(pi)[ch // 2] + ch % 2
    ne = channels // 2
    mu = np.zeros((ne, 2)) if mean is None else np.asarray(mean, np.float64).reshape(ne, 2)
    sd = np.ones((ne, 2)) if std is None else np.asarray(std, np.float64).reshape(ne, 2)
    lp = np.asarray(lprime)
    gain, bias = np.zeros((ne, 2)), np.zeros((ne, 2))
    gain[:, 0] = sign * rho * sd[lp, 0] / sd[:, 0]
    gain[:, 1] = rho * sd[lp, 1] / sd[:, 1]
    if sign < 0:
        bias[:, 0] = -(rho * mu[lp, 0] + mu[:, 0]) / sd[:, 0]
    else:
        bias[:, 0] = (rho * mu[lp, 0] - mu[:, 0]) / sd[:, 0]
    bias[:, 1] = (rho * mu[lp, 1] - mu[:, 1]) / sd[:, 1]
    src = 2 * lp[ch // 2] + ch % 2
    return gain.reshape(-1).astype(np.float32).astype(np.float64), bias.reshape(-1).astype(np.float32).astype(np.float64), src


def fuse(maps_per_member, scales, base, mirror, image_width, pi, edges=None, mean=None, std=None):
    """fuse_ref.fuse with mirrored members.  mirror: one 0/1 per member; pi: the joint permutation; edges: [E, 2], needed when next_pred
    takes part.  -> (fused, A): two triples of float64 [NB, C, H_b, W_b] arrays (None where the map took no part)."""
    import fuse_ref as F

    nm = len(maps_per_member)
    assert not mirror[base], "the base member must be unmirrored"
    s_b = float(scales[base])
    inv_m = float(np.float32(1.0) / np.float32(nm))
    lprime = mirrored_edges(edges, pi) if maps_per_member[0][2] is not None else None
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
            if mirror[m]:
                x0, x1, fx = sample_axis_mirrored(wb, a.shape[3], q, float(image_width - 1) * float(scales[m]))
                gain, bias, src = mirror_gain_bias(k, a.shape[1], rho, pi, lprime, mean, std)
                a = a[:, src]
            else:
                x0, x1, fx = sample_axis(wb, a.shape[3], q)
                gain, bias = F.gain_bias(k, a.shape[1], rho, mean, std)
            fy, fx = fy[:, None], fx[None, :]
            a00, a01 = a[:, :, y0][:, :, :, x0], a[:, :, y0][:, :, :, x1]
            a10, a11 = a[:, :, y1][:, :, :, x0], a[:, :, y1][:, :, :, x1]
            val = (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11)
            mag = (1 - fy) * ((1 - fx) * np.abs(a00) + fx * np.abs(a01)) + fy * ((1 - fx) * np.abs(a10) + fx * np.abs(a11))
            acc = acc + (val * gain[None, :, None, None] + bias[None, :, None, None])
            a_acc = a_acc + (mag * np.abs(gain)[None, :, None, None] + np.abs(bias)[None, :, None, None])
        fused.append(acc * inv_m), bound.append(a_acc * inv_m)
    return tuple(fused), tuple(bound)


# ---- a planted pyramid with mirrored members ---------------------------------------------------------------------------------------------
def planted_mirrored_pyramid(shapes, scales, mirror, base, image_width, pi, edges, mean, std, num_joints=14, sixteen_bit=False):
    """The three people of fuse_ref.planted_pyramid (the same joints, in image pixels, drawn in the same order from the same seed) rendered
    into every member's maps at its own scale.  A mirrored member holds what the net is trained to give on the mirror image: the truth
    reflected as x -> (w - 1) - x with the joints relabelled by pi, `next_pred` of edge l = (a, c) encoded from relabelled joint a to
    relabelled joint c with edge l's own statistics — which, seen from the unmirrored scene, are the statistics of the relabelled edge.
    Asserted on the restatement alone, with planted_pyramid's margins: the fused loc_pred decodes to the planted joints, every planted joint
    is a strict 3x3 maximum of the fused `prob` by at least 1e-3, and no other cell reaches THRESHOLD.
    -> dict as planted_pyramid's: maps, fused, A, truth, joints, cells."""
    edges = np.asarray(edges).reshape(-1, 2)
    ne = edges.shape[0]
    mean = np.asarray(mean, np.float64).reshape(ne, 2)
    std = np.asarray(std, np.float64).reshape(ne, 2)
    pi = np.asarray(pi)
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
    mirrored_truth = np.zeros_like(truth)
    mirrored_truth[:, pi] = truth  # joint j of the scene is joint pi[j] of the mirror image ...
    mirrored_truth[:, :, 0] = (image_width - 1) - mirrored_truth[:, :, 0]  # ... at the reflected column
    q16 = R.round_to_bf16 if sixteen_bit else (lambda v: np.asarray(v, np.float32))
    out_edges = [[l for l in range(ne) if edges[l, 0] == j] for j in range(num_joints)]
    maps = []
    for (h, w), s, flipped in zip(shapes, scales, mirror):
        s = float(s)
        seen = mirrored_truth if flipped else truth
        prob = np.zeros((num_joints, h, w), np.float32)
        loc = np.zeros((2 * num_joints, h, w), np.float32)
        nxt = np.zeros((2 * ne, h, w), np.float32)
        px = (np.arange(w) * M.STRIDE + 4.0) / s
        py = (np.arange(h) * M.STRIDE + 4.0) / s
        radius, reach = RADIUS_NET / s_b, RADIUS_NET / s_b + 2 * M.STRIDE / s
        owner = np.full((num_joints, h, w), -1)
        for q in range(3):
            for j in range(num_joints):
                x, y = seen[q, j]
                d2 = (py[:, None] - y) ** 2 + (px[None, :] - x) ** 2
                prob[j] += (PEAKS[q] * np.maximum(0.0, 1.0 - d2 / radius ** 2) ** 2).astype(np.float32)
                for r in np.nonzero(np.abs(py - y) <= reach)[0]:
                    for c in np.nonzero(np.abs(px - x) <= reach)[0]:
                        assert owner[j, r, c] < 0, "two people's neighbourhoods of joint %d overlap" % j
                        owner[j, r, c] = q
                        lt, _ = M.encode_targets(seen[q, j], seen[q, j], (r, c), s, (0, 0), (1, 1))
                        loc[2 * j:2 * j + 2, r, c] = lt
                        for l in out_edges[j]:
                            _, nt = M.encode_targets(seen[q, j], seen[q, edges[l, 1]], (r, c), s, mean[l], std[l])
                            nxt[2 * l:2 * l + 2, r, c] = nt
        maps.append(tuple(q16(a)[None] for a in (prob, loc, nxt)))
    fused, bound = fuse(maps, scales, base, mirror, image_width, pi, edges, mean, std)
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


# ---- what tests/test_flip_host.py and tests/test_gpu_flip.py share -----------------------------------------------------------------------
IMAGE_HW = (200, 261)                 # a width that is no multiple of 8: (w - 1) s is not cell-aligned
SCALES = (0.7, 1.0, 0.7, 1.0)         # two plain members, then their mirrors; base = the plain scale 1.0
MIRROR = (0, 0, 1, 1)
BASE = 1
_scene = {}


def planted(sixteen_bit):
    """The planted mirrored pyramid of a 200 x 261 image: computed once per process, never written to."""
    if sixteen_bit not in _scene:
        import caffe

        shapes = [tuple(v // 8 for v in caffe.canvas_size(IMAGE_HW[0], IMAGE_HW[1], s)) for s in SCALES]
        _scene[sixteen_bit] = planted_mirrored_pyramid(shapes, SCALES, MIRROR, BASE, IMAGE_HW[1], MIRROR_MPII14, R.all_pairs_edges(), MEAN, STD,
                                                       sixteen_bit=sixteen_bit)
    return _scene[sixteen_bit]

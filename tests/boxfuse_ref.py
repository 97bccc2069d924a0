"""Float64 NumPy restatement of the fusion rule of dc_group_decode_boxes / dc_group_decode_pose (test helper, never on the product path):
tests/flip_ref.py's `fuse` with the reflected column's `ws` given per (member, image) instead of once per member, and the restricted
decode of the box entry on the fused maps.  `sample_axis`, `sample_axis_mirrored`, `mirror_gain_bias`, `gain_bias`, `worst_ratio` and
`BOUND` are fuse_ref's and flip_ref's own.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn decodes every scale on its own and keeps the best one (estimate_pose.py:119-126),
fuses no maps and mirrors nothing, so there is no reference output to hold the rule to.  What is restated here is the definition in
include/deepcut_hip.h.

The bound is flip_ref's: a per-image `ws` changes which cells a mirrored member is sampled at, not how many roundings the sample costs,
so |device - restatement| <= BOUND * A = 16 * 2^-24 * A element by element."""
import numpy as np

import flip_ref as FL
import fuse_ref as F
from flip_ref import MIRROR_MPII14, worst_ratio  # noqa: F401  (shared with the tests)


def box_ws(boxes, scales, pyramid):
    """-> float64 [M][n]: ws[m][i] = (cw_i - 1) * (scales[i] * pyramid[m]), the inner product being the scale member m ran box i at."""
    boxes = np.asarray(boxes).reshape(-1, 4)
    scales = np.broadcast_to(np.asarray(scales, np.float64), (boxes.shape[0],))
    return np.array([[float(int(x1) - int(x0) - 1) * (float(s) * float(p)) for (x0, _y0, x1, _y1), s in zip(boxes, scales)] for p in pyramid])


def fuse(maps_per_member, scales, base, mirror, ws, pi):
    """flip_ref.fuse of `prob` and `loc_pred` with ws [M][NB]: image b of a mirrored member m is sampled at the column
    u = ((ws[m][b] - (8c + 4) q) - 4) / 8, clamped to the member's whole map.  maps_per_member: per member a (prob, loc_pred[, None])
    pair of [NB, C, H_m, W_m] arrays.  -> (fused, A): two pairs of float64 [NB, C, H_b, W_b] arrays."""
    nm = len(maps_per_member)
    assert not mirror[base], "the base member must be unmirrored"
    s_b = float(scales[base])
    inv_m = float(np.float32(1.0) / np.float32(nm))
    fused, bound = [], []
    for k in range(2):
        nb = maps_per_member[base][k].shape[0]
        hb, wb = maps_per_member[base][k].shape[2:]
        acc = a_acc = 0.0
        for m in range(nm):
            a = np.asarray(maps_per_member[m][k], np.float64)
            q = 1.0 if m == base else float(scales[m]) / s_b
            rho = 1.0 if m == base else s_b / float(scales[m])
            y0, y1, fy = F.sample_axis(hb, a.shape[2], q)
            fy = fy[:, None]
            if mirror[m]:
                gain, bias, src = FL.mirror_gain_bias(k, a.shape[1], rho, pi, None, None, None)
                a = a[:, src]
            else:
                gain, bias = F.gain_bias(k, a.shape[1], rho, None, None)
            val, mag = np.zeros((nb, a.shape[1], hb, wb)), np.zeros((nb, a.shape[1], hb, wb))
            for b in range(nb):
                if mirror[m]:
                    x0, x1, fx = FL.sample_axis_mirrored(wb, a.shape[3], q, float(ws[m][b]))
                else:
                    x0, x1, fx = F.sample_axis(wb, a.shape[3], q)
                fx = fx[None, :]
                a00, a01 = a[b][:, y0][:, :, x0], a[b][:, y0][:, :, x1]
                a10, a11 = a[b][:, y1][:, :, x0], a[b][:, y1][:, :, x1]
                val[b] = (1 - fy) * ((1 - fx) * a00 + fx * a01) + fy * ((1 - fx) * a10 + fx * a11)
                mag[b] = (1 - fy) * ((1 - fx) * np.abs(a00) + fx * np.abs(a01)) + fy * ((1 - fx) * np.abs(a10) + fx * np.abs(a11))
            acc = acc + (val * gain[None, :, None, None] + bias[None, :, None, None])
            a_acc = a_acc + (mag * np.abs(gain)[None, :, None, None] + np.abs(bias)[None, :, None, None])
        fused.append(acc * inv_m), bound.append(a_acc * inv_m)
    return tuple(fused), tuple(bound)


def box_poses(prob, loc_pred, boxes, scales, base_scale):
    """The restricted decode of the box entry on (fused) maps over the base member's canvas: pose i =
    `pose.estimate_pose.box_pose_from_maps` at scales[i] * base_scale.  -> float64 [n, 5, J]."""
    from pose.estimate_pose import box_pose_from_maps

    boxes = np.asarray(boxes).reshape(-1, 4)
    scales = np.broadcast_to(np.asarray(scales, np.float64), (boxes.shape[0],))
    return np.stack([box_pose_from_maps(prob[i], loc_pred[i], boxes[i], float(scales[i]) * float(base_scale)) for i in range(boxes.shape[0])])

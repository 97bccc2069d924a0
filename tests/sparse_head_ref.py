"""The rule of the sparse pairwise head (include/deepcut_hip.h, dc_net_pairwise_at) in NumPy float64: the 1x1 skip convolution plus
nine masked matmuls, one per tap of the stride-2 3x3 deconvolution, each on the rows and columns whose parity selects the tap.  Pinned to
oracle.OracleNet (and through it to the reference's deconvolution) by tests/test_sparse_head_host.py; the yardstick of
tests/test_gpu_sparse_pairwise.py."""
import numpy as np


def head_prototxt(n, k5, k3, h5, w5, h, w, joints=2, pairs=None, bias=True, oh=0, ow=0):
    """A head-only net: inputs x5 [n, k5, h5, w5] and x3 [n, k3, h, w], then the reference's three heads (deconvolution of x5, cropped at
    (oh, ow), plus a 1x1 skip of x3) at small widths."""
    pairs = joints * (joints - 1) if pairs is None else pairs
    out = ['name: "heads"', 'input: "x5"', "input_shape { dim: %d dim: %d dim: %d dim: %d }" % (n, k5, h5, w5), 'input: "x3"',
           "input_shape { dim: %d dim: %d dim: %d dim: %d }" % (n, k3, h, w)]
    b = "" if bias else " bias_term: false"
    for suffix, nout, crop, top in (("pose", joints, "crop1", "fc_pose"), ("locref", 2 * joints, "crop_locref", "loc_pred"),
                                    ("next", 2 * pairs, "crop_next", "next_pred")):
        up, skip = "x5_up_" + suffix, "x3_" + suffix
        out.append('layer { name: "%s" type: "Deconvolution" bottom: "x5" top: "%s" convolution_param { num_output: %d kernel_size: 3 pad: 0 '
                   'stride: 2%s } }' % (up, up, nout, b))
        out.append('layer { name: "%s" type: "Convolution" bottom: "x3" top: "%s" convolution_param { num_output: %d kernel_size: 1 pad: 0 '
                   'stride: 1%s } }' % (skip, skip, nout, b))
        out.append('layer { name: "%s" type: "Crop" bottom: "%s" bottom: "%s" top: "%sc" crop_param { offset_height: %d offset_width: %d } }'
                   % (crop, up, skip, up, oh, ow))
        out.append('layer { name: "%s" type: "Eltwise" bottom: "%s" bottom: "%sc" top: "%s" }' % (top, skip, up, top))
    out.append('layer { name: "prob" type: "Sigmoid" bottom: "fc_pose" top: "prob" }')
    return "\n".join(out) + "\n"


def sparse_head_ref(x3, x5, ws, wd, bias_s=None, bias_d=None, oh=0, ow=0):
    """x3 [NB, K3, H, W], x5 [NB, K5, h5, w5], ws [C, K3] (or [C, K3, 1, 1]), wd [K5, C, 3, 3], biases [C] or None
    -> (next, S), both float64 [NB, C, H, W]: the whole map by the rule, and the sum of the absolute values of everything added into
    each element (operand products and biases): the scale of its rounding error."""
    x3, x5, wd = (np.asarray(a, np.float64) for a in (x3, x5, wd))
    ws = np.asarray(ws, np.float64).reshape(np.shape(ws)[0], -1)
    nb, _, h, w = x3.shape
    h5, w5 = x5.shape[2:]
    c = ws.shape[0]
    bias = np.zeros(c) + (0 if bias_s is None else np.asarray(bias_s, np.float64)) + (0 if bias_d is None else np.asarray(bias_d, np.float64))
    mag = np.zeros(c) + (0 if bias_s is None else np.abs(np.asarray(bias_s, np.float64))) + (0 if bias_d is None else np.abs(np.asarray(bias_d, np.float64)))
    def mm(wnk, x):  # [n, k] x [b, k, y, x] -> [b, n, y, x] (tensordot: BLAS)
        return np.tensordot(wnk, x, axes=([1], [1])).transpose(1, 0, 2, 3)

    out = mm(ws, x3) + bias[None, :, None, None]
    s = mm(np.abs(ws), np.abs(x3)) + mag[None, :, None, None]
    for ky in range(3):
        rows = [r for r in range(h) if (r + oh - ky) % 2 == 0 and 0 <= (r + oh - ky) // 2 < h5]
        for kx in range(3):
            cols = [q for q in range(w) if (q + ow - kx) % 2 == 0 and 0 <= (q + ow - kx) // 2 < w5]
            if not rows or not cols:
                continue
            src = x5[:, :, [(r + oh - ky) // 2 for r in rows]][:, :, :, [(q + ow - kx) // 2 for q in cols]]
            out[np.ix_(range(nb), range(c), rows, cols)] += mm(wd[:, :, ky, kx].T, src)
            s[np.ix_(range(nb), range(c), rows, cols)] += mm(np.abs(wd[:, :, ky, kx]).T, np.abs(src))
    return out, s


def round_to(a, dtype):
    """a rounded to the element type of a net ('f32', 'f16' or 'bf16': nearest, ties to even) and widened to float32 again."""
    a = np.asarray(a, np.float32)
    if dtype == "f16":
        return a.astype(np.float16).astype(np.float32)
    if dtype == "bf16":
        u = a.view(np.uint32).astype(np.uint64)
        u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
        return u.astype(np.uint32).view(np.float32).reshape(a.shape)
    return a

"""CPU: the host half of the unfused Winograd F(4x4,3x3) form (csrc/wino43_f32.hip, tile `wino_f43`) against first principles in NumPy.
 * dc_wino43_pack: 36 matrices U[6 i + j] = (G g G^T)[i][j], transformed in double and rounded once, each in the row-operand order of
   v_mfma_f32_16x16x4_f32 that the batched streaming multiply reads (tests/test_stream_pack.py emulates the same layout for ws1x1f);
 * the three stages — V = B^T d B per 6 x 6 patch on the dilation-phase tile grid, 36 products M[p] = V[p] U[p], Y = A^T M A — emulated in
   float32 against a float64 direct convolution.  Measured here on the res4 shape (34 x 46, 256 -> 256, post-ReLU randn input, He-scaled
   filters): max error 5.5e-5 on a range of 5.2 = 1.0e-5 x range; the GPU test's bound is 1e-4 x max(1, range) (tests/test_gpu_winograd43.py).
   The same data through F(2x2,3x3) gives 6e-7 x range and through a direct float32 sum 3e-7 x range: the price of the points +-2."""
import numpy as np
import pytest

import caffe
from f32_ref import wino43_f32  # the form as the kernels lay it out, every stage in float32, sequential products

G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)


def _mfma16(a_lanes, b_lanes):
    """one v_mfma_f32_16x16x4_f32 step: lane 16 q + r holds A[r, q] (row operand) and B[q, r] (column operand); D = A B [16, 16]"""
    A = np.zeros((16, 4))
    B = np.zeros((4, 16))
    for lane in range(64):
        A[lane % 16, lane // 16] = a_lanes[lane]
        B[lane // 16, lane % 16] = b_lanes[lane]
    return A @ B


def _u64(g):
    return np.einsum("ia,ocab,jb->ijoc", G, g.astype(np.float64), G)  # [6, 6, cout, cin]


@pytest.mark.parametrize("cout,cin", [(64, 64), (32, 128), (16, 256)])
def test_the_image_is_36_row_operands_of_G_g_Gt(cout, cin):
    rs = np.random.RandomState(cout + cin)
    g = rs.randn(cout, cin, 3, 3).astype(np.float32)
    img = caffe.wino43_pack(g)
    assert img.shape == (36, cout // 16, cin // 16, 64, 4)
    U = _u64(g).reshape(36, cout, cin)
    x = rs.randn(16, cin).astype(np.float32)  # 16 rows of V
    for p in (0, 1, 7, 20, 35):
        # rounded once from the double product, in the layout of dc_stream1x1f_pack: within one float32 ulp of this float64 product's rounding
        # (two float64 summation orders may round to neighbouring floats), where a float32 transform would be ~8 ulp off
        near = caffe.stream1x1f_pack(U[p].astype(np.float32))
        assert np.all(np.abs(img[p].astype(np.float64) - near) <= 2.0 ** -23 * np.abs(near))
        want = U[p] @ x.astype(np.float64).T  # [cout, row]
        for f in range(cout // 16):
            d = np.zeros((16, 16))
            for j in range(cin // 16):
                xv = np.stack([x[lane % 16, (lane // 16) * (cin // 4) + 4 * j:(lane // 16) * (cin // 4) + 4 * j + 4] for lane in range(64)])
                for e in range(4):
                    d += _mfma16(img[p, f, j, :, e], xv[:, e])
            assert np.allclose(d, want[f * 16:(f + 1) * 16], rtol=0, atol=1e-5 * np.abs(want).max())
    with pytest.raises(caffe.DeepcutError):
        caffe.wino43_pack(np.zeros((24, 64, 3, 3), np.float32))


def _direct64(x, g, d):
    n, cin, h, w = x.shape
    xp = np.zeros((n, cin, h + 2 * d, w + 2 * d))
    xp[:, :, d:d + h, d:d + w] = x
    out = np.zeros((n, g.shape[0], h, w))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("oc,nchw->nohw", g[:, :, ky, kx].astype(np.float64), xp[:, :, ky * d:ky * d + h, kx * d:kx * d + w])
    return out


@pytest.mark.parametrize("shape", [(1, 256, 256, 34, 46, 1), (1, 64, 32, 5, 9, 1), (2, 64, 32, 6, 7, 1), (1, 64, 32, 9, 11, 2)],
                         ids=["res4", "5x9", "batch2_6x7", "dilation2_9x11"])
def test_three_float32_stages_against_a_float64_convolution(shape):
    n, cin, cout, h, w, d = shape
    rs = np.random.RandomState(h + w)
    x = np.maximum(rs.randn(n, cin, h, w), 0).astype(np.float32)          # post-ReLU activations
    g = (rs.randn(cout, cin, 3, 3) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)  # He-scaled
    ref = _direct64(x, g, d)
    got = wino43_f32(x, g, d)
    rng = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())
    print("wino_f43 in float32 %s: max error %.3e on a range of %.3f = %.2e x range" % (shape, err, rng, err / rng))
    assert err <= 1e-4 * max(1.0, rng)

"""Host tests of tests/f32_ref.py — the float64 reference, the sequential float32 model, the Winograd emulations — and of the bound the
tight float32 tests assert: max|got - ref| <= 3 x and rms(got - ref) <= 2 x the same statistic of a sequential float32 sum.  Its power:
  * every correct ordering is ACCEPTED — chunks of 2 (a 32x32x2 MFMA chain), 4 (16x16x4) and 16, 2- and 4-way split K with the partial
    sums added in float32, numpy's float32 matmul, the C oracle's float32 GEMM, the Winograd emulations with blocked products;
  * every subtly wrong one is REJECTED, and shown to pass the former 1e-4 x range: operands rounded to 16 significant bits (a bf16
    hi + lo pair), partial sums rounded to 16 bits every 256 K elements, an F(2x2) input transform rounded to 16 bits.  Two more are
    rejected that the former bound caught already, by a factor of 1.5 to 4: operands rounded to 11 bits (tf32 / float16) at K <= 576,
    2.5e-4 .. 3.8e-4 x range, and an F(4x4) input transform rounded to 16 bits, 1.5e-4 x range (the transform's entries reach 8) — of
    them only the rejection is asserted.  Operands rounded to 19 bits are the bound's known limit: where they land is printed, not asserted;
  * on every case of the GPU tests — the same seeds and shapes, through those files' own helpers — the chunk-of-2 and chunk-of-4 models
    are inside the margins: the reference alone keeps to them on exactly the inputs the device sees (cases above M N K = 5e8 on the
    model's pixel subset).  No case had to be changed for that, the K = 64 ones included, where the last rounding is most of the error
    of model and kernel alike and both ratios sit near 1."""
import numpy as np
import pytest

import caffe
import f32_ref as F
from oracle import oracle as O

KS = [(221, 64, 64), (240, 64, 147), (221, 64, 576), (99, 128, 1152), (30, 512, 2048), (30, 512, 4608)]  # M, N, K (147: the stem's 7x7x3)
INPUTS = ["randn", "relu"]


def _operands(mnk, kind):
    M, N, K = mnk
    rs = np.random.RandomState(K + (kind == "relu"))
    x = rs.randn(M, K)
    x = (np.maximum(x, 0) if kind == "relu" else x).astype(np.float32)              # post-ReLU activations / randn
    w = (rs.randn(N, K) * np.sqrt((2.0 if kind == "relu" else 1.0) / K)).astype(np.float32)  # He- / 1/sqrt(K)-scaled filters
    return x, w, x.astype(np.float64) @ w.astype(np.float64).T, F.seq_dot32(x, w)


def _rejected(got, ref, model, label, in_the_gap=True):
    """the new bound rejects `got`; in_the_gap: and the former 1e-4 x max(1, range) took it"""
    rmax, rrms = F.f32_ratios(got, ref, model)
    old = float(np.abs(got - ref).max()) / max(1.0, float(np.abs(ref).max()))
    print("%s: %.1f x the model's maximum, %.1f x its rms; %.2e x range (former bound 1e-4: %s)" % (label, rmax, rrms, old, "passed" if old <= 1e-4 else "caught"))
    if in_the_gap:
        assert old <= 1e-4, "%s does not pass the former bound: it is not part of the gap" % label
    with pytest.raises(AssertionError):
        F.assert_f32_tight(got, ref, model, label)
    return rmax, rrms


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------
def test_seq_dot32_is_one_rounded_product_and_one_rounded_add_per_k():
    rs = np.random.RandomState(1)
    A, B = rs.randn(5, 37).astype(np.float32), rs.randn(7, 37).astype(np.float32)
    want = np.zeros((5, 7), np.float32)
    for i in range(5):
        for j in range(7):
            acc = np.float32(0)
            for k in range(37):
                acc = np.float32(acc + np.float32(A[i, k] * B[j, k]))
            want[i, j] = acc
    assert np.array_equal(F.seq_dot32(A, B), want)
    # chunks: the exact sum of a chunk rounded once, chunk sums added in float32; split K: the runs' sums added in order
    A64, B64 = A.astype(np.float64), B.astype(np.float64)
    want = np.zeros((5, 7), np.float32)
    for k0 in range(0, 40, 4):
        want = want + (A64[:, k0:k0 + 4] @ B64[:, k0:k0 + 4].T).astype(np.float32)
    assert np.array_equal(F.blocked_dot32(A, B, 4), want)
    halves = [sum(((A64[:, k0:k0 + 4] @ B64[:, k0:k0 + 4].T).astype(np.float32) for k0 in r), np.zeros((5, 7), np.float32)) for r in (range(0, 20, 4), range(20, 40, 4))]
    assert np.array_equal(F.blocked_dot32(A, B, 4, 2), halves[0] + halves[1])
    r = F.round_bits(np.array([1 + 2.0 ** -16, 1 + 3 * 2.0 ** -16, 1 + 2.0 ** -16 + 2.0 ** -23, -3.1415927, 0.0], np.float32), 16)
    assert r.tolist()[:3] == [1.0, 1 + 2.0 ** -14, 1 + 2.0 ** -15] and r[4] == 0 and abs(r[3] + 3.1415927) <= 2.0 ** -15
    assert np.array_equal(F.round_bits(A, 24), A)


@pytest.mark.parametrize("shape", [(2, 5, 7, 9, 11, 3, 1, 1, 1), (1, 3, 8, 13, 10, 7, 2, 3, 1), (2, 6, 4, 9, 8, 3, 1, 2, 2)], ids=["3x3", "stem7x7s2", "3x3d2"])
def test_conv_ref64_against_the_oracle_accumulating_in_double(shape):
    """The oracle under set_double_acc(True) rounds its float64 sum once: within half an ulp, 2^-24 |ref|, of the float64 reference"""
    n, ci, co, h, w, k, s, p, d = shape
    rs = np.random.RandomState(h)
    x, wt = rs.randn(n, ci, h, w).astype(np.float32), rs.randn(co, ci, k, k).astype(np.float32)
    ref = F.conv_ref64(x, wt, None, s, p, d)
    O.set_double_acc(True)
    try:
        got = O.conv_forward(x, wt, None, s, p, d)
    finally:
        O.set_double_acc(False)
    assert ref.dtype == np.float64 and got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref))
    # the sequential model is the same convolution (K in im2col order: channel, kernel row, kernel column), to float32 accuracy
    assert float(np.abs(F.conv_seq32(x, wt, s, p, d).reshape(ref.shape) - ref).max()) <= 1e-5 * float(np.abs(ref).max())


@pytest.mark.parametrize("shape", [(2, 5, 7, 4, 5, 3, 3, 0, 1), (1, 4, 3, 5, 4, 2, 2, 0, 1), (2, 6, 5, 3, 4, 3, 2, 0, 1)], ids=["k3s3", "k2s2", "k3s2_overlapping"])
def test_deconv_ref64_against_the_oracle_accumulating_in_double(shape):
    """Stride >= kernel: every output is ONE rounded float64 sum, within 2^-24 |ref|.  Stride 2 under a 3x3 kernel (the net's heads): the
    oracle adds up to four rounded column sums and the bias in float32 (col2im), five roundings of at most 2^-24 x the sum of magnitudes,
    which the same reference on |x|, |w|, |bias| gives"""
    n, ci, co, h, w, k, s, p, d = shape
    rs = np.random.RandomState(h + k)
    x, wt = rs.randn(n, ci, h, w).astype(np.float32), rs.randn(ci, co, k, k).astype(np.float32)
    bias = rs.randn(co).astype(np.float32) if s < k else None
    ref = F.deconv_ref64(x, wt, bias, s, p, d)
    O.set_double_acc(True)
    try:
        got = O.deconv_forward(x, wt, bias, s, p, d)
    finally:
        O.set_double_acc(False)
    assert got.shape == ref.shape
    if s >= k:
        assert np.all(np.abs(got - ref) <= 2.0 ** -24 * np.abs(ref))
    else:
        assert np.all(np.abs(got - ref) <= 5 * 2.0 ** -24 * F.deconv_ref64(np.abs(x), np.abs(wt), np.abs(bias), s, p, d))
    seq = F.deconv_seq32(x, wt, s, p, d).reshape(ref.shape)
    assert float(np.abs(F.epilogue32(seq, *F.fold_affine64(co, bias)) - ref).max()) <= 1e-5 * float(np.abs(ref).max())


def test_the_epilogue_folds_as_the_library_does_and_the_oracle_chain_agrees():
    rs = np.random.RandomState(4)
    C = 6
    acc = rs.randn(2, C, 15)
    mean, var, sf = rs.randn(C).astype(np.float32), (1 + rs.rand(C)).astype(np.float32), np.array([0.5], np.float32)
    gamma, beta, sc = rs.randn(C).astype(np.float32), rs.randn(C).astype(np.float32), rs.randn(2, C, 15).astype(np.float32)
    a, b = F.fold_affine64(C, None, (mean, var, sf), (gamma, beta))
    m, v, g, be = [t.astype(np.float64)[None, :, None] for t in (mean, var, gamma, beta)]
    want = ((acc - m / 0.5) / np.sqrt(v / 0.5 + 1e-5)) * g + be
    assert np.allclose(F.epilogue64(acc, a, b), want, rtol=1e-13, atol=1e-13)
    assert np.array_equal(F.epilogue64(acc, a, b, sc, True), np.maximum(F.epilogue64(acc, a, b) + sc, 0))
    y = O.relu_forward(O.eltwise_sum(O.scale_forward(O.batchnorm_forward(acc.astype(np.float32), mean, var, sf), gamma, beta), sc))
    assert np.allclose(y, F.epilogue64(acc.astype(np.float32), a, b, sc, True), rtol=0, atol=1e-5)
    e32 = F.epilogue32(acc.astype(np.float32), a, b, sc, True)
    assert e32.dtype == np.float32 and np.allclose(e32, y, rtol=0, atol=1e-5)
    assert F.fold_affine64(C) == (None, None) and F.epilogue32(acc.astype(np.float32)).dtype == np.float32
    a1, b1 = F.fold_affine64(C, beta)
    assert np.array_equal(a1, np.ones(C)) and np.array_equal(b1, beta.astype(np.float64))


WINO = [(1, 64, 32, 9, 11, 2), (2, 32, 48, 7, 10, 1), (1, 32, 16, 11, 20, 3), (1, 32, 16, 1, 1, 1), (1, 128, 64, 13, 17, 1)]  # n, cin, cout, h, w, dilation


def _wino_data(shape):
    n, cin, cout, h, w, d = shape
    rs = np.random.RandomState(h + w)
    x = np.maximum(rs.randn(n, cin, h, w), 0).astype(np.float32)
    g = (rs.randn(cout, cin, 3, 3) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    return x, g, F.conv_ref64(x, g, None, 1, d, d)


@pytest.mark.parametrize("shape", WINO)
def test_the_winograd_emulations_are_the_convolution(shape):
    """dilation-phase images, ragged last tiles, a single pixel: both forms against the float64 convolution at the GPU tests' former bound"""
    x, g, ref = _wino_data(shape)
    for f in (F.wino23_f32, F.wino43_f32):
        got = f(x, g, shape[5])
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert float(np.abs(got - ref).max()) <= 1e-4 * max(1.0, float(np.abs(ref).max())), f.__name__


def test_the_pixel_subset():
    assert F.pixel_subset(1, 1564, 512, 4608) is None      # fewer than 2048 pixels: all of them
    assert F.pixel_subset(2, 1000, 64, 64) is None         # M N K <= 5e8
    for n, npix, cout, K in ((2, 4690, 1024, 256), (1, 100096, 64, 147), (1, 25024, 1024, 256)):
        p = F.pixel_subset(n, npix, cout, K)
        assert n * len(p) >= 2048 and len(p) < npix and np.array_equal(p, np.unique(p))
        assert set(range(64)) <= set(p.tolist()) and set(range(npix - 64, npix)) <= set(p.tolist())
        assert np.array_equal(p, F.pixel_subset(n, npix, cout, K))  # a fixed seed
        assert n * len(p) * cout * K <= 1.01 * max(5e8, 2048.0 * cout * K + n * cout * K)


# ---- the bound's power --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("mnk", KS, ids=lambda v: "K%d" % v[2])
def test_every_correct_ordering_is_accepted(mnk, kind):
    """... and none of them is more than 10 x better than the model on the RMS: the margins are multiples of the MODEL's error, so a model
    that loses bits would slacken them without any other test noticing.  Blocking shortens the chain of roundings a sum passes through, by
    16 at the most here (chunks of 16; chunks of 4 in four runs), which is worth about the square root of that on the RMS, 1/4 — measured
    0.25 at the least; a model with operands rounded to 16 bits puts the orderings at 0.01 .. 0.1."""
    x, w, ref, model = _operands(mnk, kind)
    M, N, K = mnk
    oracle = O.conv_forward(np.ascontiguousarray(x.T).reshape(1, K, M, 1), w.reshape(N, K, 1, 1))[0, :, :, 0].T
    got = [(F.blocked_dot32(x, w, chunk, split), "chunks of %d, split K %d" % (chunk, split)) for chunk, split in ((2, 1), (4, 1), (16, 1), (4, 2), (4, 4), (2, 4))]
    for g, what in got + [(x @ w.T, "numpy's float32 matmul"), (oracle, "the C oracle's float32 GEMM")]:
        _rmax, rrms = F.assert_f32_tight(g, ref, model, "accepted: %s K = %d, %s" % (kind, K, what))
        assert rrms >= 0.1, "%s is %.3f of the model on the RMS: the model is not a float32 sum" % (what, rrms)


@pytest.mark.parametrize("kind", INPUTS)
@pytest.mark.parametrize("mnk", KS, ids=lambda v: "K%d" % v[2])
def test_every_wrong_model_passes_the_former_bound_and_is_rejected(mnk, kind):
    x, w, ref, model = _operands(mnk, kind)
    K = mnk[2]
    # the most favourable ordering for the wrong model: chunks of 4 with 4-way split K, the most accurate of the correct ones above
    r16 = _rejected(F.blocked_dot32(F.round_bits(x, 16), F.round_bits(w, 16), 4, 4), ref, model, "rejected: %s K = %d, operands rounded to 16 bits" % (kind, K))
    assert r16[0] > F.MARGIN_MAX and r16[1] > F.MARGIN_RMS  # on both statistics
    if K <= 576:
        _rejected(F.blocked_dot32(F.round_bits(x, 11), F.round_bits(w, 11), 4, 4), ref, model, "rejected: %s K = %d, operands rounded to 11 bits" % (kind, K), in_the_gap=False)
    acc = np.zeros(ref.shape, np.float32)
    for k0 in range(0, K, 256):
        acc = F.round_bits(acc + F.blocked_dot32(x[:, k0:k0 + 256], w[:, k0:k0 + 256], 4), 16)
    _rejected(acc, ref, model, "rejected: %s K = %d, partial sums rounded to 16 bits every 256 K elements" % (kind, K))
    r19 = F.f32_ratios(F.blocked_dot32(F.round_bits(x, 19), F.round_bits(w, 19), 4, 4), ref, model)
    print("the bound's limit: %s K = %d, operands rounded to 19 bits: %.2f x the model's maximum (margin %g), %.2f x its rms (margin %g)" % (
        kind, K, r19[0], F.MARGIN_MAX, r19[1], F.MARGIN_RMS))


@pytest.mark.parametrize("form", ["wino23", "wino43"])
@pytest.mark.parametrize("shape", [WINO[0], WINO[4]])
def test_winograd_blocked_products_are_accepted_and_a_16_bit_input_transform_is_rejected(shape, form):
    x, g, ref = _wino_data(shape)
    f = F.wino23_f32 if form == "wino23" else F.wino43_f32
    model = f(x, g, shape[5])
    for chunk, split in ((4, 1), (4, 2), (2, 1), (16, 1)):
        F.assert_f32_tight(f(x, g, shape[5], lambda a, b: F.blocked_dot32(a, b, chunk, split)), ref, model, "accepted: %s %s, chunks of %d, split K %d" % (form, shape, chunk, split))
    wrong = f(x, g, shape[5], lambda a, b: F.blocked_dot32(a, b, 4, 2), lambda v: F.round_bits(v, 16))
    _rejected(wrong, ref, model, "rejected: %s %s, input transform rounded to 16 bits" % (form, shape), in_the_gap=form == "wino23")


# ---- the GPU tests' own cases: the blocked models stay inside the margins on exactly the inputs the device sees ------------------------
def _blocked_inside(layer, label):
    ref = layer.ref_on_pixels()
    for chunk, split in ((2, 1), (4, 1)):
        F.assert_f32_tight(layer.model(lambda a, b: F.blocked_dot32(a, b, chunk, split)), ref, layer.model32, "%s, chunks of %d" % (label, chunk))


def _t2_cases():
    import test_gpu_layers as L

    return [pytest.param(cfg, batch, id="%s-b%d" % (L.t2_id(cfg), batch)) for cfg in L.T2 for batch in (1, 2)]


@pytest.mark.parametrize("cfg,batch", _t2_cases())
def test_blocked_models_on_the_26_configurations(cfg, batch):
    import test_gpu_layers as L

    _blocked_inside(L.t2_case(cfg, batch), "GPU case T2 %s batch %d" % (L.t2_id(cfg), batch))
    if cfg[1] == 3 and cfg[0] == "conv":  # a 3x3 row the per-shape timing may give to wino_f23
        _blocked_inside(L.t2_case(cfg, batch, "wino23"), "GPU case T2 on wino_f23 %s batch %d" % (L.t2_id(cfg), batch))


@pytest.mark.parametrize("which", ["xcd", "dilated", "xcd_wide", "dilated_wide", "deconv", "deconv_tiny"])
def test_blocked_models_on_the_forced_tile_nets(which):
    import test_gpu_tile_shapes as T

    assert set(T._SEEDS) == {"xcd", "dilated", "xcd_wide", "dilated_wide", "deconv", "deconv_tiny", "heads"}
    _blocked_inside(T._Case(caffe, which, "f32").f32_case(), "GPU case forced tiles, net %s" % which)


def _wino_cases():
    import test_gpu_winograd as W
    import test_gpu_winograd43 as W43
    import test_gpu_winograd_blocks as WB
    import test_gpu_winograd_mixed as WM

    out = [pytest.param("wino23", c, id="wino23-%s" % "x".join(str(int(v)) for v in c)) for c in sorted(set(W.CASES) | set(WB.CASES) | set(c[0] for c in WM.CASES))]
    return out + [pytest.param("wino43", c, id="wino43-%s" % "x".join(str(int(v)) for v in c)) for c in W43.CASES]


@pytest.mark.parametrize("kind,case", _wino_cases())
def test_blocked_models_on_the_winograd_cases(kind, case):
    import test_gpu_winograd as W
    import test_gpu_winograd43 as W43

    if kind == "wino23":  # (the three F(2x2) files draw a case's data the same way: test_gpu_winograd.case_data)
        weights, x = W.case_data(case)
    else:
        _proto, _out, weights, x, _ref = W43._case_data(case)
    _blocked_inside(W.wino_case(case, weights, x, kind), "GPU case %s %s" % (kind, case))


def _stream_cases():
    import test_gpu_stream1x1_f32 as S

    return S.CASES


@pytest.mark.parametrize("case", _stream_cases())
def test_blocked_models_on_the_streaming_1x1_cases(case):
    import test_gpu_stream1x1_f32 as S

    weights, inputs = S.case_data(case)
    _blocked_inside(S.f32_case(case, weights, inputs), "GPU case ws1x1f %s" % (case,))


def _stem_cases():
    import test_gpu_stem_f32 as S

    return S.STEM_CASES


@pytest.mark.parametrize("case", _stem_cases())
def test_blocked_models_on_the_stem_cases(case):
    import test_gpu_stem_f32 as S

    weights, x = S.case_data(case)
    _blocked_inside(S.f32_case(case, weights, x), "GPU case ws7x7f %s" % (case,))

"""Host tests of the float16 helpers of tests/test_gpu_fp16.py and of the bound the tight float16 tests assert,
|got - ref| <= ulp_f16(ref) + 1e-6 x range: its form (f16_ulp against numpy's spacing over every binade) and its power to reject — a
GEMM model that accumulates in float32 and rounds once meets it, a model that rounds its partial sums to float16 every 256 K
elements passes the former 2e-3 x range bound and is rejected."""
import numpy as np
import pytest

from test_gpu_fp16 import f16_operands, f16_round, f16_ulp


def test_f16_ulp_is_numpys_spacing_in_every_binade():
    bits = np.arange(0, 0x7C00, dtype=np.uint16)  # every non-negative finite float16, subnormals and zero included
    v = bits.view(np.float16)
    want = np.spacing(v[:-1]).astype(np.float64)  # (the spacing above the largest finite value is infinite: checked below)
    assert np.array_equal(f16_ulp(v[:-1].astype(np.float32)), want)
    assert np.array_equal(f16_ulp(-v[:-1].astype(np.float32)), want)
    assert f16_ulp(65504.0) == 32.0 and f16_ulp(0.0) == 2.0 ** -24 and f16_ulp(2.0 ** -14) == 2.0 ** -24 and f16_ulp(2.0 ** -13) == 2.0 ** -23
    # reals between float16 values take their binade's spacing, up to the last float32 / float64 below a power of two
    for e in range(-14, 16):
        lo, hi = 2.0 ** e, 2.0 ** (e + 1)
        for a in (lo, lo * 1.2345678, np.nextafter(np.float32(hi), np.float32(0)), np.nextafter(hi, 0.0)):
            assert f16_ulp(a) == 2.0 ** (e - 10), (e, a)
    assert f16_ulp(np.array([[1.0, -3.0], [1e-9, 1000.0]])).tolist() == [[2.0 ** -10, 2.0 ** -9], [2.0 ** -24, 2.0 ** -1]]


def test_f16_round_and_operands():
    a = np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -11 + 2.0 ** -20, 2.0 ** -14, 2.0 ** -15, -2.0 ** -14 * 0.99, 0.1, -65504.0], np.float32)
    r = f16_round(a)
    assert r.dtype == np.float32
    assert r[:3].tolist() == [1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -10]  # ties to even, above a tie upwards
    q = f16_operands(a)
    assert q.dtype == np.float32 and q.shape == a.shape
    assert q[3] == 2.0 ** -14 and q[4] == 0.0 and q[5] == 0.0  # subnormal results are flushed, the smallest normal stays
    keep = np.abs(r) >= 2.0 ** -14
    assert np.array_equal(q[keep], r[keep]) and np.array_equal(f16_round(q), q)
    x = f16_operands(np.random.RandomState(0).randn(4, 5, 6) * 1e-4)
    assert x.shape == (4, 5, 6) and ((x == 0) | (np.abs(x) >= 2.0 ** -14)).all() and (x == 0).any() and (x != 0).any()


def _f32_chain_model(x, w):
    """A correct kernel: float32 accumulation in chains of 16 K elements (one matrix instruction each), ONE rounding to float16."""
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, x.shape[1], 16):
        acc = acc + (x[:, k0:k0 + 16] @ w[:, k0:k0 + 16].T).astype(np.float32)
    return f16_round(acc)


def _f16_partials_model(x, w):
    """A subtly wrong kernel: the partial sum is rounded to float16 after every 256 K elements."""
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for k0 in range(0, x.shape[1], 256):
        acc = f16_round(acc + x[:, k0:k0 + 256] @ w[:, k0:k0 + 256].T)
    return acc


def _excess(got, ref):
    return float((np.abs(got.astype(np.float64) - ref) - (f16_ulp(ref) + 1e-6 * float(np.abs(ref).max()))).max())


@pytest.mark.parametrize("mnk", [(64, 256, 64), (33, 128, 1152), (64, 512, 2048)])
def test_the_one_ulp_bound_takes_a_float32_accumulation_and_rejects_float16_partials(mnk):
    M, N, K = mnk
    rs = np.random.RandomState(K)
    x = f16_operands(rs.randn(M, K))
    w = f16_operands(rs.randn(N, K) / np.sqrt(K))
    ref = x.astype(np.float64) @ w.astype(np.float64).T
    rng = float(np.abs(ref).max())
    good, bad = _f32_chain_model(x, w), _f16_partials_model(x, w)
    assert _excess(good, ref) <= 0, _excess(good, ref)
    # not even the half-ulp form of the bound is missed: the one-ulp form leaves the kernels a whole rounding of room
    assert float((np.abs(good - ref) - (0.5 * f16_ulp(ref) + 1e-6 * rng)).max()) <= 0
    assert float(np.abs(bad - ref).max()) <= 2e-3 * max(1.0, rng), "the wrong model passes the former bound"
    if K > 256:
        assert _excess(bad, ref) > 0, "the one-ulp bound must reject float16 partial sums at K = %d" % K
    else:
        assert np.array_equal(bad, f16_round(x @ w.T))  # a single chunk: the wrong model IS one rounding

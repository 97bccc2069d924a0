"""-m gpu: the addresses of the ws1x1f family (csrc/stream1x1_f32.hip).  A lane's offset is loop invariant; what moves with the step sits in
the request's own descriptor, whose end — (M - 1) x stride + row bytes behind the view's base — is what drops rows >= M, and a store
must stay inside its rows and its channels.  The shapes are the smallest at which that can go wrong; the bounds are those of
tests/test_gpu_stream1x1_f32.py (2e-5 x range against the CPU oracle, tests/f32_ref.py's margins against a sequential float32 sum), of
tests/test_gpu_winograd43.py (1e-4 x range) and of tests/test_gpu_stem_f32.py.

  single layers, Cout 64 (one channel slice: a range per step up to 8 steps), K = 64 / 128 / 256 / 512, plain and shortcut + ReLU:
    M = 1, 15, 16, 17, 33    a lone row, one row short of a step, a full step, one row into the second, into the third (3 steps on a grid of
                             8 workgroups: more ranges offered than steps, the others leave at once)
    M = 181                  12 steps over 8 ranges: four ranges of two steps, four of one (srem = 4), the last step 5 rows
  ... Cout 512, M = 2597 (K >= 256: 163 steps over 32 ranges, 5-6 each) / 4196 (K <= 128: 263 steps over 64 ranges, 4-5 each): the steady
    loop behind the three peeled steps, ranges of unequal length, a partial last step
  views (dc_stream1x1f_rows): x rows with 16 more floats than K, y and the shortcut as 64 channels from channel 32 of 160, in a buffer of
    more rows than M, prefilled with a sentinel: every element outside the view's channels and every row >= M keeps its bits
  batched (through wino_f43): 64 tiles (4 full steps, 4 ranges), 30 tiles (two ranges, the last step 14 rows), 144 tiles (9 steps over 8
    ranges), K = 256 at 30 tiles
  stem: a 1 x 1 image (the smallest of tests/test_gpu_stem_f32.py) and 37 x 51 (odd: requests that hang over every edge)."""
import numpy as np
import pytest

import f32_ref as F
import test_gpu_stem_f32 as stem32
import test_gpu_winograd43 as w43
from test_gpu_stem import _net_text as stem_net_text
from test_gpu_stream1x1 import _net_text
from test_gpu_stream1x1_f32 import _oracle, _run, case_data, f32_case
from test_gpu_winograd import wino_case

pytestmark = pytest.mark.gpu

KS = (64, 128, 256, 512)
SMALL_M = (1, 15, 16, 17, 33, 181)
_ref = {}  # case -> (prototxt, output blob, weights, inputs, oracle output): made once, shared by the layer and the view tests, left unchanged


def _layer(case):
    if case not in _ref:
        n, cin, cout, h, w, shortcut, relu, affine = case
        proto, out = _net_text(n, cin, cout, h, w, shortcut, relu, affine)
        weights, inputs = case_data(case)
        ref = _oracle(proto, weights, **inputs)[out]
        ref.setflags(write=False)
        _ref[case] = (proto, out, weights, inputs, ref)
    return _ref[case]


def _case(k, m, cout, epi):
    return (1, k, cout, 1, m, epi, epi, True)  # n, cin, cout, h, w, shortcut, relu, affine


def _steady_m(k):
    return 2597 if k >= 256 else 4196


def _check(got, case, label):
    proto, out, weights, inputs, ref = _layer(case)
    assert got.shape == ref.shape
    rng = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    print("%s %s: max|hip - oracle| = %.3e (bound %.3e)" % (label, case, err, 2e-5 * rng))
    assert err <= 2e-5 * rng
    ref64, model, pixels = f32_case(case, weights, inputs)
    F.assert_f32_tight(got, ref64, model, "%s: %s" % (label, case), pixels)


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "shortcut_relu"])
@pytest.mark.parametrize("k", KS)
def test_single_layers_at_the_edges_of_a_step(gpu_caffe, k, epi, monkeypatch):
    for m in SMALL_M:
        case = _case(k, m, 64, epi)
        proto, out, weights, inputs, _r = _layer(case)
        got, plan = _run(gpu_caffe, proto, weights, inputs, out, "1", monkeypatch)
        assert "ws1x1f" in plan, plan
        _check(got, case, "ws1x1f")


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "shortcut_relu"])
@pytest.mark.parametrize("k", KS)
def test_the_steady_loop_with_ranges_of_unequal_length(gpu_caffe, k, epi, monkeypatch):
    case = _case(k, _steady_m(k), 512, epi)
    proto, out, weights, inputs, _r = _layer(case)
    got, plan = _run(gpu_caffe, proto, weights, inputs, out, "1", monkeypatch)
    assert "ws1x1f" in plan, plan
    _check(got, case, "ws1x1f")


SENTINEL = np.array([0x7F7FABCD], np.uint32).view(np.float32)[0]  # a finite value no result takes; compared as bits
VIEWS = [(k, m, 64, epi) for k in KS for epi in (False, True) for m in (17, 181)] + [(256, 2597, 512, True), (64, 4196, 512, False)]


@pytest.mark.parametrize("k,m,cout,epi", VIEWS)
def test_views_keep_every_byte_outside_their_rows_and_channels(gpu_caffe, k, m, cout, epi):
    case = _case(k, m, cout, epi)
    _proto, _out, weights, inputs, ref = _layer(case)
    a, b = F.fold_layers64(cout, weights)
    c0, ys, extra = 32, cout + 96, 19  # the view: channels [32, 32 + cout) of cout + 96, in a buffer of 19 more rows than M
    x = np.full((m, k + 16), 1e30, np.float32)  # what lies beside a pixel's K channels must not be read as an operand
    x[:m, :k] = inputs["data"][0, :, 0, :].T
    y = np.full((m + extra, ys), SENTINEL, np.float32)
    resid = None
    if epi:
        resid = np.full(y.shape, np.nan, np.float32)  # a shortcut read outside the view would show
        resid[:m, c0:c0 + cout] = inputs["sc"][0, :, 0, :].T
    gpu_caffe.stream1x1f_rows(x, weights[0][2][0].reshape(cout, k), y, y_c0=c0, m=m, scale=a.astype(np.float32), shift=b.astype(np.float32), resid=resid,
                              relu=epi)
    got = np.ascontiguousarray(y[:m, c0:c0 + cout].T).reshape(ref.shape)
    _check(got, case, "ws1x1f view")
    outside = y.view(np.uint32).copy()
    outside[:m, c0:c0 + cout] = SENTINEL.view(np.uint32)
    assert (outside == SENTINEL.view(np.uint32)).all(), "rows / channels outside the view were written: %s" % (np.argwhere(outside != SENTINEL.view(np.uint32))[:8],)


@pytest.fixture
def _wino_env(monkeypatch):
    monkeypatch.setenv("DC_AUTOTUNE", "0")
    monkeypatch.setenv("DC_WINOGRAD43", "-1")
    for v in ("DC_WINOGRAD", "DC_TUNE_CACHE", "DC_WSF43_SLOTS"):
        monkeypatch.delenv(v, raising=False)


BATCHED = [(1, 64, 64, 32, 32, 1, False), (1, 64, 64, 18, 22, 1, True), (1, 128, 64, 48, 48, 1, True), (1, 256, 64, 18, 22, 1, False)]


@pytest.mark.parametrize("case", BATCHED, ids=["64_tiles", "30_tiles", "144_tiles", "30_tiles_k256"])
def test_the_batched_form_through_wino_f43(gpu_caffe, case, _wino_env):
    proto, out, weights, x, ref = w43._case_data(case)
    net = w43._net(gpu_caffe, proto, weights)
    w43._on_the_form(net, x)
    net.blobs["data"].data[...] = x
    net.forward()
    got = net.blobs[out].data.copy()
    err, bound = float(np.abs(got - ref).max()), 1e-4 * max(1.0, float(np.abs(ref).max()))
    print("wino_f43 %s: max|hip - oracle| = %.3e (bound %.3e)" % (case, err, bound))
    assert err <= bound
    ref64, model, pixels = wino_case(case, weights, x, "wino43")
    F.assert_f32_tight(got, ref64, model, "wino_f43 on the batched ws1x1f: %s" % (case,), pixels)


@pytest.mark.parametrize("case", [(1, 1, 1, True, False), (1, 37, 51, True, True)], ids=["1x1", "37x51"])
def test_the_stem_at_the_smallest_and_an_odd_image(gpu_caffe, case, monkeypatch):
    n, h, w, relu, affine = case
    proto = stem_net_text(n, h, w, relu, affine)
    weights, x = stem32.case_data(case)
    got, plan = stem32._run(gpu_caffe, proto, weights, x, "1", monkeypatch)
    assert "ws7x7f" in plan, plan
    ref = stem32._oracle(proto, weights, data=x)["conv1"]
    assert got.shape == ref.shape
    assert float(np.abs(got - ref).max()) <= 2e-5 * max(1.0, float(np.abs(ref).max()))
    ref64, model, pixels = stem32.f32_case(case, weights, x)
    F.assert_f32_tight(got, ref64, model, "ws7x7f: %s" % (case,), pixels)

"""-m gpu: DC_OPT_SPARSE_PAIRWISE — the pairwise head of a net that leaves `next_pred` out, evaluated at the cells its consumers read
(csrc/sparse_head.hip; the rule: include/deepcut_hip.h, dc_net_pairwise_at) — against the float64 restatement in
tests/sparse_head_ref.py, which tests/test_sparse_head_host.py pins to the oracle.

Synthetic ResNet-152, DC_AUTOTUNE=0, one net per shape and element type for the whole module.  Shapes: 64x64 (map 8x8); 72x88 at batch 2
(map 9x11 over a 5x6 res5c: the last row and column are even and use two taps); 200x264 at batch 2 (map 25x33, 1 650 cells: every
parity class is longer than one 128-cell pass of the kernel)."""
import numpy as np
import pytest

import caffe
import people_ref as R
import sparse_head_ref as SR
from conftest import rand_image

pytestmark = pytest.mark.gpu

STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))  # as tests/test_gpu_people.py
SHAPES = {"64x64": (64, 64, 1), "72x88": (72, 88, 2), "200x264": (200, 264, 2)}
F32_SUM = 8705 * 2.0 ** -24  # a float32 sum of at most 4 x 2048 + 512 products and a bias, every rounding at the worst end


def _all_cells(n, h, w):
    return np.array([(b, r, c) for b in range(n) for r in range(h) for c in range(w)], np.int32)


def _reference(net, dtype):
    """ref and S of the rule from the net's own res3b7 / res5c blobs (16-bit nets: their 16-bit values) and the head's parameters, the
    filters rounded to the net's element type."""
    x3, x5 = net.blobs["res3b7"].data.copy(), net.blobs["res5c"].data.copy()
    ps, pd = net.params["res3d_next"], net.params["res5c_up_next"]
    return SR.sparse_head_ref(x3, x5, SR.round_to(ps[0].data, dtype), SR.round_to(pd[0].data, dtype), ps[1].data, pd[1].data)


_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def cost_model_tiles():
    """DC_AUTOTUNE=0 for every forward of the module (clones and re-lowered plans included): the tiles are the cost model's, so the same
    input gives the same trunk bits on every executor."""
    import os

    old = os.environ.get("DC_AUTOTUNE")
    os.environ["DC_AUTOTUNE"] = "0"
    yield
    if old is None:
        del os.environ["DC_AUTOTUNE"]
    else:
        os.environ["DC_AUTOTUNE"] = old


@pytest.fixture(scope="module")
def run(gpu_caffe, synth152):
    """run(shape, dtype) -> the record of one net, made once: forward with all outputs (the dense `next_pred` = D), then the outputs narrowed
    to loc_pred and prob, the option set, the same input forwarded again and `pairwise_at` on every cell of every image; ref / S from that
    run's own blobs.  The net stays in that state."""
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152

    def make(shape, dtype="f32"):
        if (shape, dtype) in _RUNS:
            return _RUNS[shape, dtype]
        h, w, n = SHAPES[shape]
        net = gpu_caffe.Net(deepercut_prototxt(152, h, w), path, gpu_caffe.TEST, from_text=True, dtype=dtype)
        img = rand_image(12, h, w, n=n)
        dense = net.forward_batch(img, want=("next_pred",))["next_pred"].copy()
        net.set_outputs(["loc_pred", "prob"])
        net.sparse_pairwise = True
        net.forward_batch(img, want=())
        mh, mw = net.blobs["prob"].shape[2:]
        cells = _all_cells(n, mh, mw)
        sparse = net.pairwise_at(cells)
        ref, s = _reference(net, dtype)
        rec = dict(net=net, img=img, dense=dense.astype(np.float64), cells=cells, sparse=sparse, ref=ref, s=s, at=lambda a, c=cells: a[c[:, 0], :, c[:, 1], c[:, 2]])
        _RUNS[shape, dtype] = rec
        return rec

    yield make
    _RUNS.clear()


def _ratios(rec):
    assert (rec["s"] > 0).all()
    rho_dense = float((np.abs(rec["dense"] - rec["ref"]) / rec["s"]).max())
    rho_sparse = float((np.abs(rec["sparse"].astype(np.float64) - rec["at"](rec["ref"])) / rec["at"](rec["s"])).max())
    return rho_dense, rho_sparse


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_values_float32(run, shape):
    """Every cell of every image: rho_sparse = max |sparse - ref| / S <= 4 x rho_dense = 4 x max |dense next_pred - ref| / S, the dense head
    kernel of the same net on the same input being the yardstick (both are float32 sums of the same <= 8 705 terms in different orders,
    each the maximum of ~1e5 samples; a dropped tap or channel is off by >~ 1e-4 of S), and rho_dense <= 8 705 x 2^-24 so that the
    yardstick itself is sane.
    Measured on an MI355X: rho_dense / rho_sparse = 5.04e-8 / 6.32e-8 at 64x64, 6.09e-8 / 6.72e-8 at 72x88, 1.68e-7 / 7.03e-8 at 200x264."""
    rec = run(shape)
    assert rec["sparse"].shape == (len(rec["cells"]), 364) and rec["sparse"].dtype == np.float32
    rho_dense, rho_sparse = _ratios(rec)
    print("sparse pairwise %s float32: rho_dense = %.3e, rho_sparse = %.3e (bound 4 x rho_dense = %.3e)" % (shape, rho_dense, rho_sparse, 4 * rho_dense))
    assert rho_dense <= F32_SUM
    assert rho_sparse <= 4 * rho_dense


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_values_sixteen_bit_nets(run, dtype):
    """72x88 at batch 2: ref / S from the net's own 16-bit blobs and the filters rounded to the type; the result is float32 (not rounded
    to 16 bits), so the bound is that of the float32 net at this shape, 4 x its rho_dense.
    Measured on an MI355X: rho_sparse = 6.80e-8 (float16), 4.02e-8 (bfloat16); bound 2.44e-7."""
    bound = 4 * _ratios(run("72x88"))[0]
    rec = run("72x88", dtype)
    _, rho_sparse = _ratios(rec)
    print("sparse pairwise 72x88 %s: rho_sparse = %.3e (bound 4 x rho_dense of the float32 net = %.3e)" % (dtype, rho_sparse, bound))
    assert rho_sparse <= bound


def test_a_cells_value_is_the_cells(run):
    """200x264: a shuffled list, a list with duplicates, single cells and the empty list return bit-identical values per cell."""
    rec = run("200x264")
    net, cells, full = rec["net"], rec["cells"], rec["sparse"]
    rs = np.random.RandomState(3)
    perm = rs.permutation(len(cells))
    assert np.array_equal(net.pairwise_at(cells[perm]), full[perm])
    dup = rs.randint(0, len(cells), 700)
    dup[100:200] = dup[0]
    assert np.array_equal(net.pairwise_at(cells[dup]), full[dup])
    for i in (0, 1, 33, 34, len(cells) // 2 + 7, len(cells) - 1):
        assert np.array_equal(net.pairwise_at(cells[i:i + 1]), full[i:i + 1])
    empty = net.pairwise_at(np.zeros((0, 3), np.int32))
    assert empty.shape == (0, 364)


def test_borders_by_name(run):
    """72x88 (map 9x11 over a 5x6 res5c): the corner that loses the ky = 2 / kx = 2 taps, its neighbours of the other three classes, the
    even last row and column, and image 1 of the batch."""
    rec = run("72x88")
    bound = 4 * _ratios(rec)[0]
    net = rec["net"]
    assert tuple(net.blobs["prob"].shape[2:]) == (9, 11) and tuple(net.blobs["res5c"].shape[2:]) == (5, 6)
    names = [(0, 0), (0, 1), (1, 0), (1, 1), (8, 10), (8, 9), (7, 10)]
    det = np.array([(b, r, c) for b in (0, 1) for r, c in names], np.int32)
    got = net.pairwise_at(det).astype(np.float64)
    for d, v in zip(det, got):
        ref, s = rec["ref"][d[0], :, d[1], d[2]], rec["s"][d[0], :, d[1], d[2]]
        assert (np.abs(v - ref) / s).max() <= bound, tuple(d)
    assert np.abs(rec["ref"][0] - rec["ref"][1]).max() > 1e-3  # the two images differ: image 1 was read at image 1


def _people_kw(md, **more):
    return dict(scale=1.0, threshold=0.5, radius=1, max_det=md, edges=R.all_pairs_edges(), mean=MEAN, std=STD, max_cost=30.0, seed_threshold=0.6,
                max_people=32, min_joints=2, **more)


@pytest.mark.parametrize("md", [8, 64])
def test_people_on_the_sparse_net(run, md):
    """200x264 at batch 2: the cost tensor of the sparse net's assemble_people against the restated pair costs fed the same net's
    candidates and the float64 reference map: +inf in the same places, finite entries within sqrt(2) x STD.max() x delta + 1e-9 with
    delta = max |pairwise_at - ref| at the candidates' cells (the cost's derivative in a next_pred value is at most std, and a
    prediction has two); people / cand bit for bit the restated assembly on the device's own costs; three calls alike."""
    rec = run("200x264")
    net = rec["net"]
    kw = _people_kw(md)
    runs = [net.assemble_people(return_cost=True, **kw) for _ in range(3)]
    counts, dets = net.detect_parts(1.0, 0.5, 1, md)
    finite = total = 0
    for b in range(2):
        for r in runs[1:]:
            assert np.array_equal(runs[0][b]["cost"], r[b]["cost"]) and np.array_equal(runs[0][b]["people"], r[b]["people"])
            assert np.array_equal(runs[0][b]["cand"], r[b]["cand"])
        cand_cells = np.array([(b, int(dets[b, j, i, 3]), int(dets[b, j, i, 4])) for j in range(14) for i in range(int(counts[b, j]))], np.int32)
        got_at = net.pairwise_at(cand_cells).astype(np.float64)
        delta = float(np.abs(got_at - rec["ref"][b][:, cand_cells[:, 1], cand_cells[:, 2]].T).max())
        ref_cost = R.pair_costs_from_candidates(counts[b], dets[b], rec["ref"][b], kw["edges"], 1.0, MEAN, STD)
        got = runs[0][b]["cost"]
        assert np.array_equal(np.isposinf(got), np.isposinf(ref_cost)) and not np.isnan(got).any() and not np.isneginf(got).any()
        fin = np.isfinite(ref_cost)
        err = float(np.abs(got[fin] - ref_cost[fin]).max())
        bound = np.sqrt(2.0) * STD.max() * delta + 1e-9
        print("sparse people max_det %d image %d: %d candidates, delta = %.3e, max |cost - restatement| = %.3e (bound %.3e)"
              % (md, b, len(cand_cells), delta, err, bound))
        assert err <= bound
        people, cand = R.assemble(counts[b], dets[b], got, kw["max_cost"], kw["seed_threshold"], 32, 2, None)
        assert np.array_equal(runs[0][b]["cand"], cand) and np.array_equal(runs[0][b]["people"], people)
        finite += int(fin.sum())
        total += len(cand)
    assert finite > 1000 and total > 0


def test_no_candidate_no_people_and_decode_pairwise(run):
    rec = run("200x264")
    net = rec["net"]
    out = net.assemble_people(**dict(_people_kw(8), threshold=2.0))
    assert [len(o["people"]) for o in out] == [0, 0]
    det = rec["cells"][::37]
    val = net.pairwise_at(det).astype(np.float64).reshape(len(det), 182, 2)
    for scale in (1.0, 0.75):
        got = net.decode_pairwise(det, scale, MEAN, STD)
        pt = np.stack([det[:, 2] * 8.0 + 4.0, det[:, 1] * 8.0 + 4.0], -1)[:, None, :]
        assert np.abs(got - (pt + val * STD[None] + MEAN[None]) / scale).max() <= 1e-9


def test_option_off_on_the_narrowed_net_is_refused_as_before(run):
    rec = run("64x64")
    net = rec["net"]
    net.sparse_pairwise = False
    try:
        for call in (lambda: net.assemble_people(**_people_kw(8)), lambda: net.decode_pairwise(rec["cells"][:2]), lambda: net.pairwise_at(rec["cells"][:2])):
            with pytest.raises(caffe.DeepcutError) as e:
                call()
            assert e.value.code == -4
    finally:
        net.sparse_pairwise = True
    assert np.array_equal(net.pairwise_at(rec["cells"]), rec["sparse"])


def test_state_all_outputs_reshape_clone_and_a_parameter_write(run):
    """On the 72x88 net.  The option on with all outputs wanted: the dense map is read, assemble_people's bits are those with it off.  A
    reshape to another input size and back, and a clone (no second pack), answer alike.  A write to res5c_up_next through net.params
    changes the answer to the new parameters' reference."""
    rec = run("72x88")
    net, img, cells = rec["net"], rec["img"], rec["cells"]
    bound = 4 * _ratios(rec)[0]
    # a clone: same answer, the image packed once for the model
    twin = net.clone()
    assert twin.sparse_pairwise and twin.wanted_outputs == ["loc_pred", "prob"]
    twin.forward_batch(img, want=())
    assert np.array_equal(twin.pairwise_at(cells), rec["sparse"])
    assert net.stats()["sparse_packs"] == 1 and twin.stats()["sparse_packs"] == 0
    # another input size and back
    other = net.forward_batch(rand_image(4, 64, 80, n=1), want=())
    assert other == {} and net.pairwise_at(_all_cells(1, 8, 10)).shape == (80, 364)
    net.forward_batch(img, want=())
    assert np.array_equal(net.pairwise_at(cells), rec["sparse"])
    # all outputs: the dense map, the same bits with the option on and off
    net.set_outputs(None)
    net.forward_batch(img, want=())
    on = net.assemble_people(return_cost=True, **_people_kw(8))
    at_on = net.pairwise_at(cells)
    net.sparse_pairwise = False
    off = net.assemble_people(return_cost=True, **_people_kw(8))
    assert np.array_equal(at_on, net.pairwise_at(cells)) and np.array_equal(at_on.astype(np.float64), rec["at"](rec["dense"]))
    for a, b in zip(on, off):
        assert np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["people"], b["people"]) and np.array_equal(a["cand"], b["cand"])
    net.sparse_pairwise = True
    net.set_outputs(["loc_pred", "prob"])
    # a parameter write reaches the packed image.  The deconvolution's filters negated: the same products with the other sign, so the sums are
    # those of the measured yardstick in size and number and its bound holds here too (filters of one sign would add up coherently, partial
    # sums as large as S, and float32 sums of those are several times less accurate relative to S, for the dense head as well)
    w = net.params["res5c_up_next"][0].data
    saved = w.copy()
    try:
        w[...] = -saved
        net.forward_batch(img, want=())
        got = net.pairwise_at(cells).astype(np.float64)
        ref, s = _reference(net, "f32")
        assert np.abs(rec["at"](ref) - rec["at"](rec["ref"])).max() > 1e-3
        assert (np.abs(got - rec["at"](ref)) / rec["at"](s)).max() <= bound
        assert net.stats()["sparse_packs"] == 2
    finally:
        net.params["res5c_up_next"][0].data[...] = saved
        net.forward_batch(img, want=())
    assert np.array_equal(net.pairwise_at(cells), rec["sparse"])

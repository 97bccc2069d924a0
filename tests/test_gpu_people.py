"""-m gpu: dc_net_assemble_people (part candidates -> pair costs -> greedy assembly, all on the device) against the restatement in
tests/people_ref.py, which stands on oracle/multiperson.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn has no consumer of `next_pred` and no part-candidate extraction (it stops at the maps,
SURVEY F6), so there is no reference output, test or golden vector to hold these kernels to.  The oracle restates the INVERSE of the label
encoding of the reference's training layer (src/caffe/layers/pose_data_layer.cpp:686-802), and that encoding is all it is pinned to
(tests/test_multiperson_oracle.py); the grouping rule is this project's own (include/deepcut_hip.h).  What is proven here is that the
device kernels compute exactly what that restatement computes."""
import numpy as np
import pytest

import people_ref as R
from conftest import rand_image

pytestmark = pytest.mark.gpu

H, W = 200, 264
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))


@pytest.fixture(scope="module")
def net(gpu_caffe, synth152):
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    n = gpu_caffe.Net(deepercut_prototxt(152, H, W), path, gpu_caffe.TEST, from_text=True)
    n.forward_batch(rand_image(12, H, W, n=2), want=())
    return n


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x["people"], y["people"]) and np.array_equal(x["cand"], y["cand"]) for x, y in zip(a, b))


def test_pair_costs_match_the_restatement_on_a_real_forward(net):
    """Batch 2 of the 200x264 synthetic ResNet-152: the cost tensor to 1e-9 absolute (the bound of the two decoders), +inf entries in
    exactly the same places; with and without mean / std, at two scales, with edges in both directions and in one only."""
    prob, loc, nxt = (net.blobs[k].data.copy() for k in ("prob", "loc_pred", "next_pred"))
    thr, radius, md = 0.5, 1, 8
    finite = 0
    for scale in (1.0, 0.75):
        cands = [R.M.nms_candidates(prob[b], loc[b], scale, thr, radius, md) for b in range(2)]
        counts, dets = net.detect_parts(scale, thr, radius, md)
        for b in range(2):  # stage A is detect_parts' kernel: the same candidates as the oracle's, as test_gpu_multiperson.py shows
            assert np.array_equal(counts[b], cands[b][0]) and np.array_equal(dets[b][:, :, 2:], cands[b][1][:, :, 2:])
        for which, edges in (("both directions", R.all_pairs_edges()), ("one direction", R.one_direction_edges())):
            for kw in ({}, {"mean": MEAN, "std": STD}):
                out = net.assemble_people(scale, thr, radius, md, edges=edges, max_cost=30.0, seed_threshold=0.6, return_cost=True, **kw)
                for b in range(2):
                    ref = R.pair_costs_from_candidates(cands[b][0], cands[b][1], nxt[b], edges, scale, kw.get("mean"), kw.get("std"))
                    got = out[b]["cost"]
                    assert got.shape == ref.shape == (14, 14, md, md)
                    assert np.array_equal(np.isposinf(got), np.isposinf(ref))
                    assert not np.isnan(got).any() and not np.isneginf(got).any()
                    fin = np.isfinite(ref)
                    err = np.abs(got[fin] - ref[fin]).max() if fin.any() else 0.0
                    print("pair cost: scale %g, %s, %s, image %d: %d finite, max |device - restatement| = %.3e"
                          % (scale, which, "stats" if kw else "no stats", b, fin.sum(), err))
                    assert err <= 1e-9
                    assert np.array_equal(got, got.transpose(1, 0, 3, 2))  # [c][a][k][i] is the same number
                    finite += int(fin.sum())
    assert finite > 1000


@pytest.mark.parametrize("max_cost,seed,order,min_joints", [(30.0, 0.6, None, 2), (60.0, 0.55, list(range(13, -1, -1)), 2), (8.0, 0.7, None, 1)])
def test_assembly_equals_the_restatement_on_the_devices_own_costs(net, max_cost, seed, order, min_joints):
    """people / cand / n_people bit for bit: the restated assembly runs on the device's own cost tensor and candidates, so rounding is
    no source of disagreement.  Three calls, identical outputs.  (On the random maps of the synthetic net hardly any link costs less than
    8 pixels: that case keeps single-joint people, so that it still compares something.)"""
    thr, radius, md = 0.5, 1, 8
    kw = dict(scale=1.0, threshold=thr, radius=radius, max_det=md, edges=R.all_pairs_edges(), mean=MEAN, std=STD, max_cost=max_cost,
              seed_threshold=seed, max_people=32, min_joints=min_joints, joint_order=order)
    runs = [net.assemble_people(return_cost=True, **kw) for _ in range(3)]
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])
    assert all(np.array_equal(runs[0][b]["cost"], r[b]["cost"]) for r in runs[1:] for b in range(2))
    counts, dets = net.detect_parts(1.0, thr, radius, md)
    total = 0
    for b in range(2):
        people, cand = R.assemble(counts[b], dets[b], runs[0][b]["cost"], max_cost, seed, 32, min_joints, order)
        assert np.array_equal(runs[0][b]["cand"], cand)
        assert np.array_equal(runs[0][b]["people"], people)
        total += len(cand)
    assert total > 0


def _planted_net(gpu_caffe, synth152, dtype):
    """A DC_OPT_FUSE 0 net after one forward, its three output blobs then overwritten through `.data` (host-authoritative: Net::map_ref
    uploads them, in the net's own element type)."""
    from deepcut_tools import deepercut_prototxt

    path, _ = synth152
    n = gpu_caffe.Net(deepercut_prototxt(152, H, W), path, gpu_caffe.TEST, from_text=True, fuse=0, dtype=dtype)
    n.forward_batch(rand_image(3, H, W), want=())
    return n


def _plant(n, sixteen_bit):
    edges = R.all_pairs_edges()
    h, w = n.blobs["prob"].shape[2:]
    prob, loc, nxt, joints, strays = R.planted_scene(h, w, edges, MEAN, STD, 1.0, 14, sixteen_bit)
    n.blobs["prob"].data[0] = prob
    n.blobs["loc_pred"].data[0] = loc
    n.blobs["next_pred"].data[0] = nxt
    return edges, prob, loc, nxt, joints, strays


def _check_planted(n, sixteen_bit):
    edges, prob, loc, nxt, joints, strays = _plant(n, sixteen_bit)
    thr, radius, md, max_cost, seed = 0.5, 1, 8, 20.0, 0.55
    # the restatement from the maps alone, before the device is consulted: the planted grouping, decided with room to spare
    counts, dets, cost = R.pair_costs(prob, loc, nxt, edges, 1.0, thr, radius, md, MEAN, STD)
    gaps = {}
    ref_all, cand_all = R.assemble(counts, dets, cost, max_cost, seed, 32, 1, gaps=gaps)
    ref, cand = R.assemble(counts, dets, cost, max_cost, seed, 32, 2)
    print("planted scene (%s): gap between a chosen link and the best link it rules out >= %.6g, gap to max_cost >= %.6g network pixels"
          % ("16-bit values" if sixteen_bit else "float32 values", gaps["choice"], gaps["max_cost"]))
    assert gaps["choice"] >= 1e-6 and gaps["max_cost"] >= 1e-6
    assert ref.shape == (3, 14, 3) and (cand >= 0).all()
    assert np.allclose(ref[:, :, :2], joints, rtol=0, atol=1e-9)
    assert len(cand_all) == 5 and sorted((c >= 0).sum() for c in cand_all) == [1, 1, 14, 14, 14]
    singles = sorted((int(np.argmax(c >= 0)), float(p[np.argmax(c >= 0), 0]), float(p[np.argmax(c >= 0), 1]))
                     for p, c in zip(ref_all, cand_all) if (c >= 0).sum() == 1)
    assert singles == sorted(strays)
    # the device, whole chain
    kw = dict(scale=1.0, threshold=thr, radius=radius, max_det=md, edges=edges, mean=MEAN, std=STD, max_cost=max_cost, seed_threshold=seed)
    got = n.assemble_people(min_joints=2, return_cost=True, **kw)[0]
    fin = np.isfinite(cost)
    assert np.array_equal(np.isposinf(got["cost"]), np.isposinf(cost))
    print("planted scene: max |device cost - restatement| = %.3e" % np.abs(got["cost"][fin] - cost[fin]).max())
    assert np.abs(got["cost"][fin] - cost[fin]).max() <= 1e-9
    assert np.array_equal(got["cand"], cand)
    assert np.allclose(got["people"], ref, rtol=0, atol=1e-9) and np.array_equal(got["people"][:, :, 2], ref[:, :, 2])
    got_all = n.assemble_people(min_joints=1, **kw)[0]
    assert np.array_equal(got_all["cand"], cand_all)
    return n, kw, got_all


def test_planted_people_whole_chain(gpu_caffe, synth152):
    """Route: the output blobs of a DC_OPT_FUSE 0 net written through `net.blobs[...].data` (no pass-through prototxt was needed).
    Three planted people of 14 joints and two stray peaks: the strays come back as single-joint people that min_joints=2 removes.
    The restatement asserts first, from the maps alone, that every greedy choice has a gap of at least 1e-6 network pixels to the best
    link it rules out (a link of the same person or the same candidate: links that share neither stay open whichever goes first) and to
    max_cost, so a 1e-9 difference in a cost cannot flip a choice."""
    n, kw, got_all = _check_planted(_planted_net(gpu_caffe, synth152, "f32"), False)
    # limits: fewer people allowed than there are seeds -> the first max_people in creation order
    few = n.assemble_people(min_joints=1, max_people=2, **kw)[0]
    assert np.array_equal(few["cand"], got_all["cand"][:2]) and np.array_equal(few["people"], got_all["people"][:2])
    # an image with no candidate
    n.blobs["prob"].data[0] = 0
    empty = n.assemble_people(min_joints=1, return_cost=True, **kw)[0]
    assert empty["people"].shape == (0, 14, 3) and empty["cand"].shape == (0, 14) and np.isposinf(empty["cost"]).all()


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_planted_people_on_sixteen_bit_nets(gpu_caffe, synth152, dtype):
    """The same planted scene with every map value rounded to one float16 and bfloat16 hold exactly: the same grouping, and — the
    uploaded values being exact — the same costs to 1e-9."""
    n = _planted_net(gpu_caffe, synth152, dtype)
    assert n.dtype == dtype
    _check_planted(n, True)


def test_refusals(net, gpu_caffe, synth152):
    edges = R.all_pairs_edges()
    kw = dict(edges=edges, max_cost=20.0, seed_threshold=0.5)
    with pytest.raises(ValueError):
        net.assemble_people(edges=edges[:181], max_cost=20.0, seed_threshold=0.5)
    # past the Python checks: the library's own answer to a wrong n_edges is DC_ESHAPE
    import ctypes as C

    import caffe.pycaffe as pc

    q = pc.AssembleParams(1.0, 0.5, 1, 8, 20.0, 0.5, 32, 1)
    e = np.ascontiguousarray(edges[:181])
    count, people = np.zeros(2, np.int32), np.zeros((2, 32, 14, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert pc._lib.dc_net_assemble_people(net._h, C.byref(q), 181, vp(e), None, None, None, vp(count), vp(people), None, None) == -3
    assert b"181 edges" in pc._lib.dc_last_error()
    # next_pred left out by DC_OPT_OUTPUTS: DC_EUNSUP
    from deepcut_tools import deepercut_prototxt

    c = gpu_caffe.Net(deepercut_prototxt(152, H, W), synth152[0], gpu_caffe.TEST, from_text=True, want=["loc_pred", "prob"])
    c.forward_batch(rand_image(12, H, W), want=())
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        c.assemble_people(**kw)
    assert ei.value.code == -4 and "next_pred" in str(ei.value)


def test_estimate_people_on_a_uint8_image(net):
    """= forward_images + assemble_people by hand; the net's output selection is what it was."""
    from pose import estimate_people, people_boxes

    img = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
    edges = R.all_pairs_edges()
    before = net.wanted_outputs
    kw = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
    got = estimate_people(img, None, None, (edges, MEAN, STD), scale=1.0, net=net, **kw)
    assert net.wanted_outputs == before == ["loc_pred", "next_pred", "prob"]
    net.forward_images(img, 1.0, want=(), pose=False)
    by_hand = net.assemble_people(scale=1.0, edges=edges, mean=MEAN, std=STD, **kw)[0]["people"]
    assert got.shape == by_hand.shape and got.shape[1:] == (14, 3) and np.array_equal(got, by_hand)
    boxes = people_boxes(got, img.shape, 10)
    assert boxes.shape == (len(got), 4) and (boxes[:, 2] > boxes[:, 0]).all() and (boxes[:, 3] > boxes[:, 1]).all()


# ---- crowded scenes: every 256-thread loop of the two kernels past its first trip ------------------------------------------------
CROWD_SEED = 21  # chosen on the CPU: the restatement alone links some candidates and leaves others alone at max_cost 15 and 60
CROWD = dict(scale=1.0, threshold=0.5, radius=1, max_det=64, seed_threshold=0.7, max_people=256, min_joints=1)
_scenes = {}


def _crowded(kind):
    """kind: "f32", "16bit" or "lattice" -> the maps and the restatement's candidates and costs of them, computed once per process and
    never written to afterwards.  40 candidates per joint: MD * MD = 4096 cost entries per joint pair, J * MD = 896 predictions,
    people x candidates up to 10240 links."""
    if kind not in _scenes:
        edges = R.all_pairs_edges()
        prob, loc, nxt = R.crowded_scene(H // 8, W // 8, edges, CROWD_SEED, lattice=kind == "lattice", sixteen_bit=kind == "16bit")
        stats = {} if kind == "lattice" else {"mean": MEAN, "std": STD}
        counts, dets, cost = R.pair_costs(prob, loc, nxt, edges, 1.0, CROWD["threshold"], 1, CROWD["max_det"], stats.get("mean"), stats.get("std"))
        assert (counts == 40).all()
        _scenes[kind] = dict(edges=edges, prob=prob, loc=loc, nxt=nxt, counts=counts, dets=dets, cost=cost, stats=stats)
    return _scenes[kind]


@pytest.fixture(scope="module")
def crowd_net(gpu_caffe, synth152):
    return _planted_net(gpu_caffe, synth152, "f32")


def _check_crowded(n, sc, max_cost, want_ties=0, **over):
    """The assertions of the crowded scenes, for one max_cost: candidates and costs against the restatement of the maps, the assembly
    against the restatement run on the device's own candidates and costs (bit for bit), three identical runs.  -> the run's stats."""
    n.blobs["prob"].data[0], n.blobs["loc_pred"].data[0], n.blobs["next_pred"].data[0] = sc["prob"], sc["loc"], sc["nxt"]
    q = dict(CROWD, **over)
    order = q.pop("joint_order", None)
    # the restatement alone first: what the scene is there for must happen in it
    st = {}
    alone, alone_cand = R.assemble(sc["counts"], sc["dets"], sc["cost"], max_cost, q["seed_threshold"], q["max_people"], q["min_joints"], order, stats=st)
    linked, single = int((alone_cand >= 0).sum() - len(alone_cand)), int(((alone_cand >= 0).sum(1) == 1).sum())
    print("crowded scene, max_cost %g, %s: the restatement alone has %d people, %d linked joints, %d single-joint people, %d tie steps, "
          "at most %d links per joint" % (max_cost, over or "defaults", len(alone_cand), linked, single, st["tie_steps"], st["max_links"]))
    assert st["max_links"] > 256 or q["max_people"] < 256, "people x candidates never left the first trip of the 256-thread loops"
    assert st["tie_steps"] >= want_ties
    counts, dets = n.detect_parts(1.0, q["threshold"], q["radius"], q["max_det"])
    assert np.array_equal(counts[0], sc["counts"]) and np.array_equal(dets[0][:, :, 2:], sc["dets"][:, :, 2:])
    # score, cell row and cell column exactly; x and y to 1e-9, the bound the decoders are held to everywhere in this file (the device
    # evaluates cell * 8 + 4 + loc * sqrt(53) in its own order); the assembly below runs on the DEVICE's candidates, so it is not affected
    assert np.abs(dets[0][:, :, :2] - sc["dets"][:, :, :2]).max() <= 1e-9
    kw = dict(edges=sc["edges"], max_cost=max_cost, joint_order=order, **dict(q, **sc["stats"]))
    runs = [n.assemble_people(return_cost=True, **kw)[0] for _ in range(3)]
    got, fin = runs[0]["cost"], np.isfinite(sc["cost"])
    assert np.array_equal(np.isposinf(got), np.isposinf(sc["cost"])) and not np.isnan(got).any() and not np.isneginf(got).any()
    err = float(np.abs(got[fin] - sc["cost"][fin]).max())
    print("crowded scene: %d finite costs, max |device - restatement| = %.3e" % (fin.sum(), err))
    assert err <= 1e-9
    assert np.array_equal(got, got.transpose(1, 0, 3, 2))
    people, cand = R.assemble(counts[0], dets[0], got, max_cost, q["seed_threshold"], q["max_people"], q["min_joints"], order)
    assert len(runs[0]["cand"]) == len(cand)  # the people count
    assert np.array_equal(runs[0]["cand"], cand) and np.array_equal(runs[0]["people"], people)
    for r in runs[1:]:
        assert np.array_equal(r["cand"], cand) and np.array_equal(r["people"], people) and np.array_equal(r["cost"], got)
    return dict(st, people=len(alone_cand), linked=linked, single=single)


@pytest.mark.parametrize("max_cost", [15.0, 60.0, 1e9])
def test_crowded_scene_at_the_entry_limits(crowd_net, max_cost):
    """40 candidates per joint with max_det = 64 (kPeopleMaxDet) and max_people = 256 (kPeopleMaxPeople): the cost kernel's loops over
    MD * MD and J * MD and the assembly's loops over people x candidates take up to 40 trips, and the arg-min's per-thread part really
    compares several links.  At the two finite max_cost values some candidates link and others do not."""
    st = _check_crowded(crowd_net, _crowded("f32"), max_cost)
    assert st["max_links"] > 256
    if max_cost < 1e9:
        assert st["linked"] > 0 and st["single"] > 0, st
    else:
        # nothing is too far to link, so a person is only ever seeded by a candidate that found every person taken: joint 0 seeds its 25
        # candidates at or above the seed threshold, and later joints, with 40 candidates each, seed the rest up to 40 people
        assert st["people"] == 40 and st["single"] == 0, st


@pytest.mark.parametrize("order", [None, list(range(13, -1, -1))], ids=["default_order", "reversed_order"])
def test_lattice_scene_ties_go_to_the_first_link(crowd_net, order):
    """Every cost is a distance between points of a 16-pixel lattice, so the minimal link cost is shared by several open links at many
    steps (counted by the restatement: at least 10): the winner must be the first in (person, candidate) order, through the per-thread
    part of the arg-min (e ascending within a thread) and through the LDS reduction (the smaller e of two equal costs)."""
    st = _check_crowded(crowd_net, _crowded("lattice"), 40.0, want_ties=10, joint_order=order)
    assert st["tie_steps"] >= 10 and st["max_links"] > 256


def test_crowded_scene_under_the_caps(crowd_net):
    """max_people = 24, below the 25 seeds of the first joint, and min_joints = 14 (only complete people stay)."""
    few = _check_crowded(crowd_net, _crowded("f32"), 60.0, max_people=24)
    assert few["people"] == 24
    whole = _check_crowded(crowd_net, _crowded("f32"), 1e9, min_joints=14)
    assert 0 < whole["people"] < 40


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_crowded_scene_on_sixteen_bit_nets(gpu_caffe, synth152, dtype):
    """The crowded scene with every map value rounded to one that float16 and bfloat16 hold exactly (round_to_bf16; the 40 scores of a
    joint are distinct such values): the same assertions."""
    n = _planted_net(gpu_caffe, synth152, dtype)
    assert n.dtype == dtype
    st = _check_crowded(n, _crowded("16bit"), 60.0)
    assert st["max_links"] > 256 and st["linked"] > 0

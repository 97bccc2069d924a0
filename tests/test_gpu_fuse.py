"""-m gpu: dc_group_fuse_maps / dc_group_detect_parts / dc_group_assemble_people (the maps of a pyramid fused on the device, then the
people assembly on the fused maps) against the restatement in tests/fuse_ref.py and, behind it, tests/people_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and combines nothing across scales, so there is no
reference output, test or golden vector to hold the fusion to.  The rule is this project's own (include/deepcut_hip.h); what is proven
here is that the device computes what its restatement computes, within the float32 bound the restatement derives (16 * 2^-24 * A)."""
import numpy as np
import pytest

import fuse_ref as F
import people_ref as R
from fuse_ref import MEAN, SCALES, STD, match_people, planted

pytestmark = pytest.mark.gpu

IMG = np.random.RandomState(31).randint(0, 256, (2, 88, 120, 3)).astype(np.uint8)
PYRAMID = (1.0, 0.7, 1.3)  # canvases 88x120, 64x88, 120x160: maps 11x15, 8x11, 15x20 — one member finer, one coarser than member 0
ALL = ("prob", "loc_pred", "next_pred")


def _group(caffe, path, image_hw, scales, n=1, **kw):
    from deepcut_tools import deepercut_prototxt

    shapes = [(n,) + tuple(caffe.canvas_size(image_hw[0], image_hw[1], s)) for s in scales]
    net = caffe.Net(deepercut_prototxt(152, shapes[0][1], shapes[0][2], n), path, caffe.TEST, from_text=True, **kw)
    return caffe.NetGroup.for_shapes(net, shapes)


@pytest.fixture(scope="module")
def forwarded(gpu_caffe, synth152):
    """The float32 group after ONE grouped forward of IMG over PYRAMID, and the maps that forward returned (never written to)."""
    grp = _group(gpu_caffe, synth152[0], IMG.shape[1:3], PYRAMID, n=2)
    outs = grp.forward_images(IMG, PYRAMID, want=ALL, pose=False)
    return grp, [tuple(o[k].copy() for k in ALL) for o in outs]


def _check_fusion(grp, maps, what):
    assert [m[0].shape[2:] for m in maps] == [(11, 15), (8, 11), (15, 20)]
    for base in (0, 1):
        ref, a = F.fuse(maps, PYRAMID, base, MEAN, STD)
        got = grp.fuse_maps(PYRAMID, base, MEAN, STD)
        again = grp.fuse_maps(PYRAMID, base, MEAN, STD)
        for k, name in enumerate(ALL):
            assert got[name].dtype == np.float32 and got[name].shape == ref[k].shape
            ratio = F.worst_ratio(got[name], ref[k], a[k])
            print("%s, base %d, %s: worst |device - restatement| / (16 * 2^-24 * A) = %.4f" % (what, base, name, ratio))
            assert ratio <= 1.0
            assert np.array_equal(got[name], again[name])


def test_fused_maps_of_a_real_forward_match_the_restatement(forwarded):
    """Batch 2, three scales, canvases that overhang the image (so the coarser member's samples are clamped at the far edges and the
    finer member's at the near ones), base = the first and then the second member."""
    grp, maps = forwarded
    _check_fusion(grp, maps, "float32")
    # a subset of the maps: the same numbers, and nothing else is written
    part = grp.fuse_maps(PYRAMID, 1, want=("prob", "loc_pred"))
    full = grp.fuse_maps(PYRAMID, 1, MEAN, STD)
    assert sorted(part) == ["loc_pred", "prob"] and all(np.array_equal(part[k], full[k]) for k in part)
    # one map alone: its rows of the table start at channel 0, whichever maps would have come before it
    for name in ALL:
        one = grp.fuse_maps(PYRAMID, 1, MEAN, STD, want=(name,))
        assert list(one) == [name] and np.array_equal(one[name], full[name]), name


@pytest.mark.parametrize("kw", [dict(dtype="f16"), dict(dtype="bf16"), dict(fuse=0)], ids=["f16", "bf16", "fuse0"])
def test_fused_maps_on_sixteen_bit_and_unfused_members(gpu_caffe, synth152, kw):
    """float16 / bfloat16 members: their maps come back as the exact float32 of the 16-bit values the kernel reads, so the same bound
    holds.  DC_OPT_FUSE 0 members: the three maps are separate tensors, not channel views of the merged head tensor."""
    grp = _group(gpu_caffe, synth152[0], IMG.shape[1:3], PYRAMID, n=2, **kw)
    outs = grp.forward_images(IMG, PYRAMID, want=ALL, pose=False)
    _check_fusion(grp, [tuple(o[k] for k in ALL) for o in outs], "+".join("%s=%s" % i for i in kw.items()))


def test_one_member_fuses_to_its_own_maps(gpu_caffe, synth152):
    grp = _group(gpu_caffe, synth152[0], IMG.shape[1:3], (0.7,), n=2)
    grp.forward_images(IMG, (0.7,), want=(), pose=False)
    got = grp.fuse_maps((0.7,), 0, MEAN, STD)
    for k in ALL:
        mine = grp.nets[0].blobs[k].data
        assert got[k].shape == mine.shape and np.array_equal(got[k].view(np.uint32), np.ascontiguousarray(mine, np.float32).view(np.uint32)), k


def _same(a, b):
    return all(np.array_equal(x["people"], y["people"]) and np.array_equal(x["cand"], y["cand"]) and np.array_equal(x["cost"], y["cost"])
               for x, y in zip(a, b))


@pytest.mark.parametrize("base", [0, 1])
def test_chain_on_the_devices_own_fused_maps(forwarded, base):
    """detect_parts and assemble_people of the group against the oracle's candidates and the restated costs and assembly run on the
    maps fuse_maps returned (the float32 values the chain reads): the standard tests/test_gpu_people.py holds the single net to."""
    grp, _ = forwarded
    fused = grp.fuse_maps(PYRAMID, base, MEAN, STD)
    thr, radius, md, max_cost, seed = 0.5, 1, 8, 40.0, 0.55
    edges = R.all_pairs_edges()
    kw = dict(threshold=thr, radius=radius, max_det=md, edges=edges, mean=MEAN, std=STD, max_cost=max_cost, seed_threshold=seed, max_people=32,
              min_joints=1)
    runs = [grp.assemble_people(PYRAMID, base, return_cost=True, **kw) for _ in range(3)]
    assert _same(runs[0], runs[1]) and _same(runs[0], runs[2])
    counts, dets = grp.detect_parts(PYRAMID, base, thr, radius, md)
    total = finite = 0
    for b in range(2):
        ref_counts, ref_dets = R.M.nms_candidates(fused["prob"][b], fused["loc_pred"][b], PYRAMID[base], thr, radius, md)
        assert np.array_equal(counts[b], ref_counts) and np.array_equal(dets[b][:, :, 2:], ref_dets[:, :, 2:])
        assert np.allclose(dets[b][:, :, :2], ref_dets[:, :, :2], rtol=0, atol=1e-9)
        ref_cost = R.pair_costs_from_candidates(ref_counts, ref_dets, fused["next_pred"][b], edges, PYRAMID[base], MEAN, STD)
        got = runs[0][b]["cost"]
        assert np.array_equal(np.isposinf(got), np.isposinf(ref_cost)) and not np.isnan(got).any()
        fin = np.isfinite(ref_cost)
        err = float(np.abs(got[fin] - ref_cost[fin]).max()) if fin.any() else 0.0
        print("fused chain, base %d, image %d: %d candidates, %d finite costs, max |device - restatement| = %.3e" % (base, b, counts[b].sum(), fin.sum(), err))
        assert err <= 1e-9
        people, cand = R.assemble(counts[b], dets[b], got, max_cost, seed, 32, 1)
        assert np.array_equal(runs[0][b]["cand"], cand) and np.array_equal(runs[0][b]["people"], people)
        total += len(cand)
        finite += int(fin.sum())
    assert total > 0 and finite > 0


def _planted_group(gpu_caffe, synth152, dtype):
    """A DC_OPT_FUSE 0 net and two clones after one grouped forward of a 200 x 264 image over SCALES; the members' output blobs are then
    overwritten through `.data` (host-authoritative: Net::map_ref uploads them in the members' own element type)."""
    grp = _group(gpu_caffe, synth152[0], (200, 264), SCALES, fuse=0, dtype=dtype)
    img = np.random.RandomState(8).randint(0, 256, (200, 264, 3)).astype(np.uint8)
    grp.forward_images(img, SCALES, want=(), pose=False)
    return grp


@pytest.mark.parametrize("dtype,sixteen_bit", [("f32", False), ("bf16", True)])
def test_planted_pyramid_whole_chain(gpu_caffe, synth152, dtype, sixteen_bit):
    """Three planted people rendered into every member's maps at its own scale, base = the middle scale.  The restatement decides from
    the maps alone, with room to spare (tests/test_fuse_host.py asserts the gaps), which candidates there are and how they group; the
    device returns exactly that `cand`, and every joint within sqrt(53) / s_b times the float32 bound of the fused loc_pred."""
    sc = planted(sixteen_bit)
    grp = _planted_group(gpu_caffe, synth152, dtype)
    assert grp.nets[0].dtype == dtype
    for net, maps in zip(grp.nets, sc["maps"]):
        for k, name in enumerate(ALL):
            assert net.blobs[name].shape[2:] == maps[k].shape[2:]
            net.blobs[name].data[...] = maps[k]
    edges = R.all_pairs_edges()
    fused = [a[0] for a in sc["fused"]]
    counts, dets, cost, people, cand = F.assemble_fused(fused, edges, SCALES[1], MEAN, STD)
    got = grp.assemble_people(SCALES, 1, threshold=F.THRESHOLD, radius=1, max_det=8, edges=edges, mean=MEAN, std=STD, max_cost=20.0,
                              seed_threshold=0.5, min_joints=2)[0]
    assert np.array_equal(got["cand"], cand) and (cand >= 0).all() and cand.shape == (3, 14)
    who = match_people(got["people"], sc["joints"])
    assert sorted(who) == [0, 1, 2]
    worst = 0.0
    for p, q in enumerate(who):
        for j in range(14):
            r, c = sc["cells"][q][j]
            for k in range(2):
                lim = R.M.LOCREF / SCALES[1] * F.BOUND * sc["A"][1][0, 2 * j + k, r, c] + 1e-12  # (+ the double arithmetic of the decode)
                err = abs(got["people"][p, j, k] - sc["joints"][q, j, k])
                worst = max(worst, err / lim)
                assert err <= lim, (q, j, k, err, lim)
    print("planted pyramid (%s): worst joint error / bound = %.4f" % (dtype, worst))
    dev = grp.fuse_maps(SCALES, 1, MEAN, STD)
    for k, name in enumerate(ALL):
        assert F.worst_ratio(dev[name], sc["fused"][k], sc["A"][k]) <= 1.0, name


def test_estimate_people_over_a_pyramid(gpu_caffe, synth152):
    """estimate_people(scales=[...]) = NetGroup.forward_images + NetGroup.assemble_people by hand (base: the scale nearest 1.0);
    estimate_people(scale=s) is what it was: Net.forward_images + Net.assemble_people."""
    from deepcut_tools import deepercut_prototxt
    from pose import estimate_people
    from pose.estimate_pose import _scale_group

    net = gpu_caffe.Net(deepercut_prototxt(152, 88, 120), synth152[0], gpu_caffe.TEST, from_text=True)
    img = np.random.RandomState(4).randint(0, 256, (85, 115, 3)).astype(np.uint8)
    edges = R.all_pairs_edges()
    kw = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
    scales = [1.3, 1.0, 1.0]
    got = estimate_people(img, None, None, (edges, MEAN, STD), net=net, scales=scales, **kw)
    assert net.wanted_outputs == ["loc_pred", "next_pred", "prob"]
    grp = _scale_group(net, 3)
    grp.forward_images(img, scales, want=(), pose=False)
    by_hand = grp.assemble_people(scales, 1, edges=edges, mean=MEAN, std=STD, **kw)[0]["people"]
    assert got.shape == by_hand.shape and got.shape[1:] == (14, 3) and np.array_equal(got, by_hand)
    other = grp.assemble_people(scales, 0, edges=edges, mean=MEAN, std=STD, **kw)[0]["people"]
    assert np.array_equal(estimate_people(img, None, None, (edges, MEAN, STD), net=net, scales=scales, base=0, **kw), other)
    # one scale, as before
    single = estimate_people(img, None, None, (edges, MEAN, STD), scale=0.8, net=net, **kw)
    net.forward_images(img, 0.8, want=(), pose=False)
    assert np.array_equal(single, net.assemble_people(scale=0.8, edges=edges, mean=MEAN, std=STD, **kw)[0]["people"])
    with pytest.raises(ValueError):
        estimate_people(img, None, None, (edges, MEAN, STD), scale=0.8, net=net, scales=scales, **kw)


def test_next_pred_left_out_by_a_member(gpu_caffe, synth152):
    """DC_OPT_OUTPUTS without next_pred on the members: DC_EUNSUP where next_pred is asked for or needed; prob and loc_pred still fuse."""
    grp = _group(gpu_caffe, synth152[0], IMG.shape[1:3], PYRAMID, n=2, want=["loc_pred", "prob"])
    outs = grp.forward_images(IMG, PYRAMID, want=("prob", "loc_pred"), pose=False)
    for call in (lambda: grp.fuse_maps(PYRAMID, 0, MEAN, STD),
                 lambda: grp.assemble_people(PYRAMID, 0, edges=R.all_pairs_edges(), mean=MEAN, std=STD, max_cost=20.0)):
        with pytest.raises(gpu_caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == -4 and "next_pred" in str(ei.value)
    maps = [(o["prob"], o["loc_pred"], None) for o in outs]
    ref, a = F.fuse(maps, PYRAMID, 0)
    got = grp.fuse_maps(PYRAMID, 0, want=("prob", "loc_pred"))
    for k, name in enumerate(("prob", "loc_pred")):
        assert F.worst_ratio(got[name], ref[k], a[k]) <= 1.0
    counts, dets = grp.detect_parts(PYRAMID, 0, 0.5, 1, 8)
    for b in range(2):
        ref_counts, ref_dets = R.M.nms_candidates(got["prob"][b], got["loc_pred"][b], PYRAMID[0], 0.5, 1, 8)
        assert np.array_equal(counts[b], ref_counts) and np.array_equal(dets[b][:, :, 2:], ref_dets[:, :, 2:])


def test_device_destinations_on_a_callers_stream_then_the_groups_own(forwarded):
    """dc_group_fuse_maps into device buffers, asynchronous on a caller's stream, followed at once by calls on the group's own stream
    with another base: the later calls wait (an event) for the first one's work before they reuse the group's fused buffer, so both
    results are what they are alone."""
    import ctypes as C

    import torch

    import caffe.pycaffe as pc

    grp, _ = forwarded
    want = [grp.fuse_maps(PYRAMID, base, MEAN, STD) for base in (0, 1)]
    counts_want, dets_want = grp.detect_parts(PYRAMID, 1, 0.5, 1, 8)
    st = torch.cuda.Stream()
    dev = {k: torch.empty(want[0][k].shape, device="cuda") for k in ALL}
    sc = np.ascontiguousarray(PYRAMID, np.float64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    for _ in range(3):
        rc = pc._lib.dc_group_fuse_maps(grp._h, vp(sc), 0, 182, vp(np.ascontiguousarray(MEAN)), vp(np.ascontiguousarray(STD)),
                                        C.c_void_p(dev["prob"].data_ptr()), C.c_void_p(dev["loc_pred"].data_ptr()),
                                        C.c_void_p(dev["next_pred"].data_ptr()), 1, C.c_void_p(st.cuda_stream))
        assert rc == 0, pc._lib.dc_last_error()
        own = grp.fuse_maps(PYRAMID, 1, MEAN, STD)
        counts, dets = grp.detect_parts(PYRAMID, 1, 0.5, 1, 8)
        st.synchronize()
        assert all(np.array_equal(dev[k].cpu().numpy(), want[0][k]) for k in ALL)
        assert all(np.array_equal(own[k], want[1][k]) for k in ALL)
        assert np.array_equal(counts, counts_want) and np.array_equal(dets, dets_want)

"""-m gpu: stage D of the people assembly, the completion pass (complete_kernel, csrc/people.hip; the rule: include/deepcut_hip.h,
dc_complete_params), against the float64 restatement in tests/complete_ref.py, through every entry that assembles people.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps; like stages B and C the rule is this project's own, and what is
proven here is that the device computes what the restatement computes.

Everything runs on the 200 x 264 synthetic ResNet-152 of tests/test_gpu_people.py (maps of 25 x 33 cells), DC_AUTOTUNE=0.  The device
floors e * scale / 8 where e is a mean it sums in its own rounding, so every comparison first looks at how close the restatement's
e * scale / 8 came to an integer: the planted cases assert a distance >= 1e-6, the random maps leave such items out (at most 1 %)."""
import numpy as np
import pytest

import complete_ref as D
import people_ref as R
from conftest import rand_image

pytestmark = pytest.mark.gpu

H, W = 200, 264
EDGES = R.all_pairs_edges()
MEAN, STD = D.MEAN, D.STD
# the random maps of the synthetic net are smooth, scores between 0.16 and 0.85: this mix leaves joints missing for each of the reasons
# (on the CPU oracle's maps of the same input: 642 items, 259 fills, 143 below fill_threshold, 240 short of predictors)
REAL = dict(threshold=0.5, radius=1, max_det=8, max_cost=40.0, seed_threshold=0.55, max_people=32, min_joints=2)
REAL_FILL = dict(fill_threshold=0.6, fill_radius=3, min_support=3)
_nets = {}


@pytest.fixture(scope="module", autouse=True)
def cost_model_tiles():
    """DC_AUTOTUNE=0 for every forward of the module: nothing is timed, and every executor of a model runs the same tiles."""
    import os

    old = os.environ.get("DC_AUTOTUNE")
    os.environ["DC_AUTOTUNE"] = "0"
    yield
    if old is None:
        del os.environ["DC_AUTOTUNE"]
    else:
        os.environ["DC_AUTOTUNE"] = old
    _nets.clear()


def _net(kind, caffe, path):
    """Once per module.  "planted:<dtype>": a DC_OPT_FUSE 0 net after one batch-2 forward, whose output blobs the tests overwrite through
    `.data`; "real": a forward of two random images; "sparse": the same narrowed to loc_pred and prob, with the sparse pairwise head."""
    from deepcut_tools import deepercut_prototxt

    if kind not in _nets:
        proto = deepercut_prototxt(152, H, W)
        if kind.startswith("planted:"):
            n = caffe.Net(proto, path, caffe.TEST, from_text=True, fuse=0, dtype=kind.split(":")[1])
            n.forward_batch(rand_image(3, H, W, n=2), want=())
        else:
            kw = dict(want=["loc_pred", "prob"], sparse_pairwise=True) if kind == "sparse" else {}
            n = caffe.Net(proto, path, caffe.TEST, from_text=True, **kw)
            n.forward_batch(rand_image(12, H, W, n=2), want=())
        _nets[kind] = n
    return _nets[kind]


@pytest.fixture(scope="module")
def planted(gpu_caffe, synth152):
    return _net("planted:f32", gpu_caffe, synth152[0])


@pytest.fixture(scope="module")
def real(gpu_caffe, synth152):
    return _net("real", gpu_caffe, synth152[0])


def _plant(n, sc, image=0):
    n.blobs["prob"].data[image] = sc["prob"]
    n.blobs["loc_pred"].data[image] = sc["loc"]
    n.blobs["next_pred"].data[image] = sc["nxt"]


def _clear(n, image):
    n.blobs["prob"].data[image] = 0


def _equal(got, want, wcand, skip=()):
    """cand, "filled" and scores exactly, x and y to 1e-9 (the bound the decoders are held to everywhere): the chosen cell is the
    restatement's.  skip: (person, joint) pairs left out."""
    keep = np.ones(wcand.shape, bool)
    for q, j in skip:
        keep[q, j] = False
    assert got["cand"].shape == wcand.shape and got["people"].shape == want.shape
    assert np.array_equal(got["cand"][keep], wcand[keep])
    assert got["filled"].dtype == np.bool_ and np.array_equal(got["filled"], got["cand"] == -2)
    assert np.array_equal(got["people"][:, :, 2][keep], want[:, :, 2][keep])
    err = float(np.abs(got["people"][:, :, :2] - want[:, :, :2])[keep].max()) if keep.any() else 0.0
    assert err <= 1e-9, err
    return err


def _case(n, sc, image=0, fill=None, **over):
    """One planted case: the restatement from the maps alone (stages A to D), with the windows placed with room to spare, then the device's
    whole chain on the same maps.  -> (the device's dict, the restatement's items by (person, joint))."""
    _plant(n, sc, image)
    dets, people, cand = D.assemble_scene(sc, **over)
    items = []
    want, wcand = D.complete_scene(sc, dets, people, cand, items=items, **(fill or {}))
    assert D.smallest_margin(items) >= 1e-6
    q = dict(D.ASSEMBLY, **over)
    got = n.assemble_people(scale=1.0, edges=sc["edges"], mean=MEAN, std=STD, complete=dict(D.FILL, **(fill or {})), **q)[image]
    _equal(got, want, wcand)
    return got, {(it["q"], it["j"]): it for it in items}


def _whole_chain(n, sixteen_bit):
    sc = D.lowered_scene(sixteen_bit)
    _clear(n, 1)
    got, items = _case(n, sc)
    assert sorted(items) == sorted(D.LOWERED) and all(it["cell"] == sc["cells"][k] for k, it in items.items())
    assert got["cand"].shape == (3, 14) and sorted((int(q), int(j)) for q, j in zip(*np.nonzero(got["filled"]))) == sorted(D.LOWERED)
    for q, j in D.LOWERED:
        assert got["people"][q, j, 2] == 0.3125 and np.abs(got["people"][q, j, :2] - sc["joints"][q, j]).max() <= 1e-9
    # the joints stage C assigned: the bits of the call without completion
    kw = dict(scale=1.0, edges=sc["edges"], mean=MEAN, std=STD, **D.ASSEMBLY)
    plain = n.assemble_people(**kw)[0]
    assert "filled" not in plain and n.completion is None
    held = plain["cand"] >= 0
    assert np.array_equal(held, ~got["filled"]) and np.array_equal(got["cand"][held], plain["cand"][held])
    assert np.array_equal(got["people"][held], plain["people"][held]) and (plain["people"][~held] == 0).all() and (plain["cand"][~held] == -1).all()
    return sc, kw, plain, got


def test_planted_scene_whole_chain(planted):
    """The scene of tests/test_complete_host.py through assemble_people(complete=...): the three lowered joints come back at the planted
    points, everything else is the call without completion, bit for bit; three calls, one result; the setting on the net does the same."""
    sc, kw, plain, got = _whole_chain(planted, False)
    for _ in range(2):
        again = planted.assemble_people(complete=D.FILL, **kw)[0]
        assert all(np.array_equal(again[k], got[k]) for k in ("people", "cand", "filled"))
    planted.completion = D.FILL
    try:
        as_state = planted.assemble_people(**kw)[0]
        off_once = planted.assemble_people(complete=False, **kw)[0]
        assert planted.completion == D.FILL
    finally:
        planted.completion = None
    assert all(np.array_equal(as_state[k], got[k]) for k in ("people", "cand", "filled"))
    assert "filled" not in off_once and np.array_equal(off_once["people"], plain["people"]) and np.array_equal(off_once["cand"], plain["cand"])


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_planted_scene_on_sixteen_bit_nets(gpu_caffe, synth152, dtype):
    """The same with every map value rounded to one float16 and bfloat16 hold exactly (0.3125 is one)."""
    n = _net("planted:" + dtype, gpu_caffe, synth152[0])
    assert n.dtype == dtype
    _whole_chain(n, True)


def _same_result(a, b, keys=("people", "cand", "cost")):
    return len(a) == len(b) and all(np.array_equal(x[k], y[k]) for x, y in zip(a, b) for k in keys)


def test_off_is_off(planted, real):
    """completion None, and completion enabled with a fill_threshold above every score (the launch runs and fills nothing): people, cand
    and cost are the bits of the call without it.  (The library counts no launches of the assembly — dc_net_stats and the plan cover the
    forward — so that no launch is added shows here only as: the result carries no "filled".)"""
    sc = D.lowered_scene()
    _plant(planted, sc)
    _clear(planted, 1)
    for n, q in ((planted, D.ASSEMBLY), (real, REAL)):
        kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, return_cost=True, **q)
        assert n.completion is None
        base = n.assemble_people(**kw)
        assert all("filled" not in d for d in base) and sum(len(d["cand"]) for d in base) > 0
        assert any((d["cand"] == -1).any() for d in base)
        assert _same_result(n.assemble_people(complete=None, **kw), base)
        high = n.assemble_people(complete=dict(fill_threshold=2.0, fill_radius=16, min_support=1), **kw)
        assert _same_result(high, base) and all(not d["filled"].any() for d in high)
        assert n.completion is None


# ---- window geometry, each case on the planted net -----------------------------------------------------------------------------------
def _aimed(sc, q, j, target_xy, peak=0.3125):
    """A copy of the scene in which every held joint of person q predicts joint j at target_xy (image pixels), the joint's own dim peak
    is gone and — peak not None — a peak of that score stands on the target's cell, if that is on the map."""
    out = dict(sc, prob=sc["prob"].copy(), nxt=sc["nxt"].copy())
    lut = R.edge_table(sc["edges"])
    for a in range(14):
        if a == j:
            continue
        l = lut[a, j]
        r, c = sc["cells"][q, a]
        _, nt = R.M.encode_targets(sc["joints"][q, a], target_xy, (r, c), 1.0, MEAN[l], STD[l])
        out["nxt"][2 * l:2 * l + 2, r, c] = nt
    r, c = sc["cells"][q, j]
    out["prob"][j, r, c] = 0
    tr, tc = int(np.floor(target_xy[1] / 8)), int(np.floor(target_xy[0] / 8))
    if peak is not None and 0 <= tr < 25 and 0 <= tc < 33:
        out["prob"][j, tr, tc] = peak
    return out


def test_fill_radius_zero_counts_the_expected_cell_only(planted):
    sc = D.lowered_scene()
    _clear(planted, 1)
    got, items = _case(planted, sc, fill=dict(fill_radius=0))
    assert got["filled"].sum() == 3  # a hit: every dim peak stands on the cell its person expects it on
    r, c = sc["cells"][0, 3]
    off = dict(sc, prob=sc["prob"].copy())
    off["prob"][3, r, c], off["prob"][3, r, c + 1] = 0, 0.3125  # one cell off: a miss
    got, items = _case(planted, off, fill=dict(fill_radius=0))
    assert got["cand"][0, 3] == -1 and (got["people"][0, 3] == 0).all() and got["filled"].sum() == 2
    got, items = _case(planted, off, fill=dict(fill_radius=1))
    assert got["cand"][0, 3] == -2 and items[0, 3]["cell"] == (r, c + 1)


def test_fill_radius_sixteen_clipped_window_of_several_trips(planted):
    """fill_radius 16 on the 25 x 33 map: 33 rows never fit, so the window is clipped above and below for every item; a 33-column
    window fits this map exactly when its centre is column 16, so no window can lose columns on both sides here: person 0 (columns 4-5)
    loses them on the left, person 2 (columns 27-29) on the right.  25 x 21 cells or more: nine trips of 64 lanes and more.  The choice
    is the window's maximum outside the exclusion zones: a brighter value far from the expected cell, in the last trip's rows, wins over
    the dim peak next to it, and the other people's held peaks, brighter still, are never taken."""
    sc = D.lowered_scene(lowered=((0, 6), (2, 7)))  # rows 11 and 12 or so: 16 rows up and 16 down both leave the map
    far = dict(sc, prob=sc["prob"].copy())
    far["prob"][6, 24, 19] = 0.4375   # inside person 0's window (columns 0..20 at least), bottom row
    far["prob"][7, 23, 13] = 0.4375   # inside person 2's window (columns 12..32 at least)
    far["prob"][7, 0, 2] = 0.46875    # outside it: never seen
    _clear(planted, 1)
    got, items = _case(planted, far, fill=dict(fill_radius=16))
    assert items[0, 6]["cell"] == (24, 19) and items[2, 7]["cell"] == (23, 13)
    for (q, j), left in (((0, 6), True), ((2, 7), False)):
        row0, col0 = int(items[q, j]["e"][1] // 8), int(items[q, j]["e"][0] // 8)
        assert row0 - 16 < 0 and row0 + 16 > 24
        assert (col0 - 16 < 0) == left and (col0 + 16 > 32) == (not left)
    assert got["people"][0, 6, 2] == 0.4375 and got["people"][2, 7, 2] == 0.4375
    # without the far values the dim peaks are the maxima outside the zones
    got, items = _case(planted, sc, fill=dict(fill_radius=16))
    assert items[0, 6]["cell"] == sc["cells"][0, 6] and items[2, 7]["cell"] == sc["cells"][2, 7]


@pytest.mark.parametrize("target,cell", [((5.3, 3.7), (0, 0)), ((32 * 8 + 3.3, 24 * 8 + 5.1), (24, 32))], ids=["first_cell", "last_cell"])
def test_expected_cell_in_a_corner_of_the_map(planted, target, cell):
    sc = _aimed(D.lowered_scene(), 0, 3, target)
    _clear(planted, 1)
    got, items = _case(planted, sc)
    assert items[0, 3]["cell"] == cell and got["cand"][0, 3] == -2 and got["people"][0, 3, 2] == 0.3125
    # ... and found from two cells away, through the clipped window
    moved = dict(sc, prob=sc["prob"].copy())
    moved["prob"][3, cell[0], cell[1]] = 0
    near = (2, 2) if cell == (0, 0) else (22, 30)
    moved["prob"][3, near[0], near[1]] = 0.3125
    got, items = _case(planted, moved)
    assert items[0, 3]["cell"] == near
    got, items = _case(planted, moved, fill=dict(fill_radius=1))
    assert got["cand"][0, 3] == -1


def test_expected_position_off_the_map(planted):
    """By less than fill_radius cells: what is left of the window is searched.  By more: the joint stays missing."""
    base = D.lowered_scene()
    r = base["cells"][0, 3][0]
    _clear(planted, 1)
    for x, found in ((-8.5, True), (-30.0, False)):  # expected column -2 and -4, fill_radius 2
        sc = _aimed(base, 0, 3, (x, r * 8 + 4.3), peak=None)
        sc["prob"][3, r, 0] = 0.3125
        got, items = _case(planted, sc)
        assert (got["cand"][0, 3] == -2) == found and (items[0, 3]["cell"] == (r, 0)) == found
        assert items[0, 3]["why"] == (None if found else "off the map")
    for y, found in ((25 * 8 + 7.5, True), (27 * 8 + 2.5, False)):  # expected row 25 and 27 of 25 rows
        sc = _aimed(base, 0, 3, (44.2, y), peak=None)
        sc["prob"][3, 24, 5] = 0.3125
        got, items = _case(planted, sc)
        assert (got["cand"][0, 3] == -2) == found and items[0, 3]["why"] == (None if found else "off the map")


def test_ties_nan_scores_and_nan_predictions(planted):
    base = D.lowered_scene()
    r, c = base["cells"][0, 3]
    _clear(planted, 1)
    sc = dict(base, prob=base["prob"].copy())
    sc["prob"][3, r - 1, c + 1] = 0.3125  # equal scores: one at a lower row-major index than the dim peak ...
    sc["prob"][3, r + 1, c - 1] = 0.3125  # ... one at a higher
    got, items = _case(planted, sc)
    assert items[0, 3]["cell"] == (r - 1, c + 1)
    sc["prob"][3, r - 2, c - 2] = np.nan  # a NaN in the window, at the lowest index of all: ignored
    sc["prob"][3, r + 2, c + 2] = np.nan
    got, items = _case(planted, sc)
    assert items[0, 3]["cell"] == (r - 1, c + 1) and not np.isnan(got["people"]).any()
    # a NaN next_pred at a held cell, on an edge into the missing joint: the joint stays missing, the person's other fill does not care
    sc = dict(base, nxt=base["nxt"].copy())
    r7, c7 = base["cells"][0, 7]
    sc["nxt"][2 * R.edge_table(EDGES)[7, 3], r7, c7] = np.nan
    got, items = _case(planted, sc)
    assert items[0, 3]["why"] == "not finite" and got["cand"][0, 3] == -1 and got["cand"][0, 9] == -2 and got["cand"][1, 5] == -2


def test_an_empty_image_and_a_single_person_share_a_call(planted):
    one = D.lowered_scene()
    one["prob"] = one["prob"].copy()
    one["prob"][:, :, 10:] = 0  # person 0 alone (columns 4-5); the strays go too
    _clear(planted, 0)
    got, items = _case(planted, one, image=1)
    assert got["cand"].shape == (1, 14) and sorted(items) == [(0, 3), (0, 9)] and got["filled"].sum() == 2
    both = planted.assemble_people(scale=1.0, edges=EDGES, mean=MEAN, std=STD, complete=D.FILL, **D.ASSEMBLY)
    assert both[0]["people"].shape == (0, 14, 3) and both[0]["cand"].shape == (0, 14) and both[0]["filled"].shape == (0, 14)
    assert np.array_equal(both[1]["cand"], got["cand"])


def test_max_people_two_of_three_planted(planted):
    """The third person is never made, so the candidates of its joints are held by nobody and exclude nothing."""
    sc = D.lowered_scene()
    _clear(planted, 1)
    got, items = _case(planted, sc, max_people=2)
    assert got["cand"].shape == (2, 14) and sorted(items) == sorted(D.LOWERED) and got["filled"].sum() == 3


# ---- real forwards: the restatement on the device's own candidates, people and maps ----------------------------------------------------
def _compare_with_restatement(label, base, got, dets, maps, next_of, scale, fill, radius=1):
    """base / got: the entry's results without and with completion; dets [n, J, MD, 5] from detect_parts; maps: prob, loc_pred [n, ...]
    as downloaded; next_of(b, cand, dets) -> what complete_ref takes as `nxt`.  Items whose e * scale / 8 lies within 1e-6 of an integer
    are left out (at most 1 %).  -> (items, fills)"""
    total = skipped = fills = 0
    worst = 0.0
    reasons = {}
    for b in range(len(base)):
        assert np.array_equal(got[b]["cand"] >= 0, base[b]["cand"] >= 0)
        held = base[b]["cand"] >= 0
        assert np.array_equal(got[b]["cand"][held], base[b]["cand"][held]) and np.array_equal(got[b]["people"][held], base[b]["people"][held])
        items = []
        want, wcand = D.complete(dets[b], base[b]["people"], base[b]["cand"], maps["prob"][b], maps["loc_pred"][b],
                                 next_of(b, base[b]["cand"], dets[b]), EDGES, MEAN, STD, scale, radius, items=items, **fill)
        skip = [(it["q"], it["j"]) for it in items if it["margin"] < 1e-6]
        worst = max(worst, _equal(got[b], want, wcand, skip))
        total, skipped, fills = total + len(items), skipped + len(skip), fills + int((wcand == -2).sum())
        for it in items:
            reasons[it["why"] or "filled"] = reasons.get(it["why"] or "filled", 0) + 1
    print("%s: %d items, %d left out (e * scale / 8 within 1e-6 of an integer), %d fills, max |x, y - restatement| = %.3e; %r"
          % (label, total, skipped, fills, worst, reasons))
    assert skipped <= 0.01 * total
    return total, fills


def test_real_forward_batch_two(real):
    """Random maps of the synthetic net, batch 2.  Three identical calls, three identical results."""
    maps = {k: real.blobs[k].data.copy() for k in ("prob", "loc_pred", "next_pred")}
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **REAL)
    base = real.assemble_people(**kw)
    runs = [real.assemble_people(complete=REAL_FILL, **kw) for _ in range(3)]
    assert _same_result(runs[0], runs[1], ("people", "cand", "filled")) and _same_result(runs[0], runs[2], ("people", "cand", "filled"))
    counts, dets = real.detect_parts(1.0, REAL["threshold"], REAL["radius"], REAL["max_det"])
    total, fills = _compare_with_restatement("real forward", base, runs[0], dets, maps, lambda b, cand, d: maps["next_pred"][b], 1.0, REAL_FILL)
    assert fills >= 50
    # a wide window at another scale, predictors from one joint on
    wide = dict(fill_threshold=0.7, fill_radius=16, min_support=1)
    kw = dict(kw, scale=0.75)
    base = real.assemble_people(**kw)
    got = real.assemble_people(complete=wide, **kw)
    counts, dets = real.detect_parts(0.75, REAL["threshold"], REAL["radius"], REAL["max_det"])
    _compare_with_restatement("real forward, scale 0.75, radius 16", base, got, dets, maps, lambda b, cand, d: maps["next_pred"][b], 0.75, wide)


def test_sparse_pairwise(gpu_caffe, synth152):
    """A net narrowed to loc_pred and prob with the sparse pairwise head: the restatement reads `next_pred` at the held candidates'
    cells from Net.pairwise_at, which is what stage D reads there."""
    n = _net("sparse", gpu_caffe, synth152[0])
    assert n.wanted_outputs == ["loc_pred", "prob"] and n.sparse_pairwise
    maps = {k: n.blobs[k].data.copy() for k in ("prob", "loc_pred")}
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **REAL)
    base = n.assemble_people(**kw)
    got = n.assemble_people(complete=REAL_FILL, **kw)
    counts, dets = n.detect_parts(1.0, REAL["threshold"], REAL["radius"], REAL["max_det"])

    def next_of(b, cand, d):
        cells = sorted(set((int(d[j, cand[q, j], 3]), int(d[j, cand[q, j], 4])) for q, j in zip(*np.nonzero(cand >= 0))))
        values = n.pairwise_at([(b, r, c) for r, c in cells])
        return {cell: values[i] for i, cell in enumerate(cells)}

    total, fills = _compare_with_restatement("sparse pairwise", base, got, dets, maps, next_of, 1.0, REAL_FILL)
    assert fills >= 50


@pytest.mark.parametrize("flip", [False, True], ids=["pyramid", "pyramid_and_mirror"])
def test_fused_pyramid_and_mirror(gpu_caffe, synth152, flip):
    """NetGroup.assemble_people(complete=...) on two scales, and on the same two with their mirrors: the restatement runs on the maps
    fuse_maps returns and on the group's own candidates."""
    from deepcut_tools import deepercut_prototxt
    from pose.people import MIRROR_MPII14

    img = np.random.RandomState(37).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    scales = (1.0, 0.7, 1.0, 0.7) if flip else (1.0, 0.7)
    mkw = dict(mirror=(0, 0, 1, 1), image_width=W, joint_mirror=MIRROR_MPII14) if flip else {}
    shapes = [(2,) + tuple(gpu_caffe.canvas_size(H, W, s)) for s in scales]
    net = gpu_caffe.Net(deepercut_prototxt(152, shapes[0][1], shapes[0][2], 2), synth152[0], gpu_caffe.TEST, from_text=True)
    grp = gpu_caffe.NetGroup.for_shapes(net, shapes)
    grp.forward_images(img, scales, want=(), pose=False, mirror=mkw.get("mirror"))
    fused = grp.fuse_maps(scales, 0, MEAN, STD, edges=EDGES if flip else None, **mkw)
    kw = dict(edges=EDGES, mean=MEAN, std=STD, **dict(REAL, **mkw))
    base = grp.assemble_people(scales, 0, **kw)
    got = grp.assemble_people(scales, 0, complete=REAL_FILL, **kw)
    assert grp.completion is None and all(m.completion is None for m in grp.nets)
    counts, dets = grp.detect_parts(scales, 0, REAL["threshold"], REAL["radius"], REAL["max_det"], **mkw)
    total, fills = _compare_with_restatement("fused " + ("pyramid + mirror" if flip else "pyramid"), base, got, dets, fused,
                                             lambda b, cand, d: fused["next_pred"][b], scales[0], REAL_FILL)
    assert fills > 0
    # the group's own setting does the same, and a member's is not read
    grp.nets[0].completion = dict(fill_threshold=0.2)
    grp.completion = REAL_FILL
    as_state = grp.assemble_people(scales, 0, **kw)
    assert _same_result(as_state, got, ("people", "cand", "filled"))
    grp.completion = None
    assert _same_result(grp.assemble_people(scales, 0, **kw), base, ("people", "cand"))


# ---- tracker, async entry, frames in flight --------------------------------------------------------------------------------------------
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(6)]
CHAIN = dict(edges=EDGES, mean=MEAN, std=STD, threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)


def _sync_loop(caffe, net, frames, complete):
    tracker = caffe.Tracker(n_joints=14, **TKW)
    out = []
    for f in frames:
        net.forward_images(f, 1.0, want=(), pose=False)
        out.append(net.track_people(tracker, scale=1.0, complete=complete, **CHAIN)[0])
    return out, tracker


def _same_frame(got, want, keys=("people", "cand", "filled", "ids", "place")):
    return all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in keys)


def test_tracker_receives_the_completed_people(real, gpu_caffe):
    """track_people(complete=...) returns assemble_people(complete=...)'s people bit for bit, and its ids are those Tracker.update gives
    on these people — not on the people without completion, whose holes the tracker would have compared."""
    chained, by_hand = gpu_caffe.Tracker(n_joints=14, **TKW), gpu_caffe.Tracker(n_joints=14, **TKW)
    total = 0
    try:
        for k in range(3):
            real.forward_images(FRAMES[k], 1.0, want=(), pose=False)
            want = real.assemble_people(scale=1.0, complete=REAL_FILL, **CHAIN)[0]
            got = real.track_people(chained, scale=1.0, complete=REAL_FILL, **CHAIN)[0]
            assert _same_frame(got, want, ("people", "cand", "filled")) and got["filled"].any()
            m = len(want["people"])
            ids, place = by_hand.update([want["people"]])
            assert np.array_equal(ids[0, :m], got["ids"]) and np.array_equal(place[0, :m], got["place"])
            total += m
    finally:
        real.forward_batch(rand_image(12, H, W, n=2), want=())  # the module's other tests read this net's first forward
    a, b = chained.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a) and total > 0
    # the tracks hold the filled joints of the last frame
    poses = a["poses"].reshape(-1, 3)
    assert any((poses == row).all(1).any() for row in want["people"][got["filled"]])


def test_async_entry_and_frames_in_flight(gpu_caffe, synth152):
    """track_frames_async(...).result() and a VideoPipeline of depth 2 over six frames give what the synchronous loop gives, bit for
    bit, with completion on: as an argument of every request, and as the net's setting, which the pipeline's clone copies."""
    from deepcut_tools import VideoPipeline, deepercut_prototxt

    net = gpu_caffe.Net(deepercut_prototxt(152, H, W), synth152[0], gpu_caffe.TEST, from_text=True)
    want, by_hand = _sync_loop(gpu_caffe, net, FRAMES, REAL_FILL)
    assert sum(int(w["filled"].sum()) for w in want) > 0 and net.completion is None
    tracker = gpu_caffe.Tracker(n_joints=14, **TKW)
    got = [net.track_frames_async(f, tracker, 1.0, complete=REAL_FILL, **CHAIN).result()[0] for f in FRAMES]
    assert all(_same_frame(g, w) for g, w in zip(got, want)) and net.completion is None
    a, b = tracker.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    plain = net.track_frames_async(FRAMES[0], None, 1.0, **CHAIN).result()[0]
    assert set(plain) == {"people", "cand"}
    for as_state in (False, True):
        tracker = gpu_caffe.Tracker(n_joints=14, **TKW)
        net.completion = REAL_FILL if as_state else None
        pipe = VideoPipeline(net, tracker, depth=2, stats=(EDGES, MEAN, STD), choose_streams=False,
                             complete=None if as_state else REAL_FILL, **{k: v for k, v in CHAIN.items() if k not in ("edges", "mean", "std")})
        assert [m.completion for m in pipe.nets] == [net.completion] * 2
        for k, f in enumerate(FRAMES):
            pipe.submit(f, tag=k)
        out = pipe.drain()
        net.completion = None
        assert [t for t, _, _ in out] == list(range(6))
        for (_, people, ids), w in zip(out, want):
            assert np.array_equal(people, w["people"]) and np.array_equal(ids, w["ids"])

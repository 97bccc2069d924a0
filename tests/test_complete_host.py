"""Stage D of the people assembly (completion) without a GPU: the float64 restatement of tests/complete_ref.py on planted scenes, and
the refusals of dc_net_set_completion / dc_group_set_completion, which need no device.

PARITY UNPINNED BY THE REFERENCE: the reference repository stops at the maps; the rule (include/deepcut_hip.h, dc_complete_params) is
this project's own, like stages B and C."""
import ctypes as C

import numpy as np
import pytest

import complete_ref as D
import people_ref as R


@pytest.fixture(scope="module")
def scene():
    sc = D.lowered_scene()
    sc["dets"], sc["people"], sc["cand"] = D.assemble_scene(sc)
    return sc


def test_the_assembly_leaves_the_lowered_joints_missing_and_completion_fills_them(scene):
    sc = scene
    people, cand = sc["people"], sc["cand"]
    assert cand.shape == (3, 14)
    missing = sorted((int(q), int(j)) for q, j in zip(*np.nonzero(cand < 0)))
    assert missing == sorted(D.LOWERED)
    items = []
    got, gcand = D.complete_scene(sc, sc["dets"], people, cand, items=items)
    assert sorted((it["q"], it["j"]) for it in items) == sorted(D.LOWERED)
    margin = D.smallest_margin(items)
    print("planted scene: smallest distance of e * scale / 8 to an integer = %.6g" % margin)
    assert margin >= 1e-6  # the device's rounding of e cannot move a window
    for it in items:
        assert it["support"] == 13 - sum(1 for q, j in D.LOWERED if q == it["q"] and j != it["j"])
        assert it["cell"] == sc["cells"][it["q"], it["j"]] and it["why"] is None
    # filled at the planted points, with the lowered score; nothing else changes
    for q, j in D.LOWERED:
        assert gcand[q, j] == -2 and got[q, j, 2] == 0.3125
        assert np.abs(got[q, j, :2] - sc["joints"][q, j]).max() <= 1e-9
    keep = cand >= 0
    assert np.array_equal(gcand[keep], cand[keep]) and np.array_equal(got[keep], people[keep])
    assert np.array_equal(gcand < 0, cand < 0) and (gcand[~keep] == -2).all()
    # the inputs are not written to
    assert (cand[~keep] == -1).all() and (people[~keep] == 0).all()


def _why(sc, people, cand, **over):
    items = []
    got, gcand = D.complete_scene(sc, sc["dets"], people, cand, items=items, **over)
    return items, got, gcand


def test_one_predictor_is_not_enough_for_min_support_two(scene):
    cand = np.full((1, 14), -1, np.int32)
    cand[0, 0] = scene["cand"][0, 0]
    people = np.zeros((1, 14, 3))
    people[0, 0] = scene["people"][0, 0]
    items, got, gcand = _why(scene, people, cand, min_support=2)
    assert len(items) == 13 and all(it["support"] == 1 and it["why"] == "support" for it in items)
    assert np.array_equal(gcand, cand) and np.array_equal(got, people)
    # ... and is with min_support 1: the joints whose peaks stand are found (the three lowered ones included, for person 0)
    items, got, gcand = _why(scene, people, cand, min_support=1)
    assert all(it["cell"] == scene["cells"][0, it["j"]] for it in items) and (gcand[0, 1:] == -2).all()


def test_no_edge_into_the_joint():
    """one_direction_edges lists a -> c with a < c only: nothing points at joint 0."""
    sc = D.lowered_scene(edges=R.one_direction_edges(), lowered=((2, 0), (1, 5)))  # (the last person: the order of seeding stays)
    sc["dets"], people, cand = D.assemble_scene(sc)
    assert sorted((int(q), int(j)) for q, j in zip(*np.nonzero(cand < 0))) == [(1, 5), (2, 0)]
    items, got, gcand = _why(sc, people, cand)
    by = {(it["q"], it["j"]): it for it in items}
    assert by[2, 0]["support"] == 0 and by[2, 0]["why"] == "support" and gcand[2, 0] == -1 and (got[2, 0] == 0).all()
    assert by[1, 5]["support"] == 5 and gcand[1, 5] == -2  # joints 0..4 point at 5


def _with_next(scene, change):
    sc = dict(scene, nxt=scene["nxt"].copy())
    lut = R.edge_table(sc["edges"])
    change(sc["nxt"], lut)
    return sc


def test_expected_position_off_the_map(scene):
    """Every predictor of (0, 3) sends it 1000 standard deviations to the left: more than fill_radius cells off the map."""
    def change(nxt, lut):
        for a in range(14):
            if a != 3:
                r, c = scene["cells"][0, a]
                nxt[2 * lut[a, 3], r, c] = -1000.0

    sc = _with_next(scene, change)
    items, got, gcand = _why(sc, scene["people"], scene["cand"])
    by = {(it["q"], it["j"]): it for it in items}
    assert by[0, 3]["why"] == "off the map" and by[0, 3]["e"][0] * 1.0 / 8 < -D.FILL["fill_radius"] - 1
    assert gcand[0, 3] == -1 and gcand[0, 9] == -2 and gcand[1, 5] == -2


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_prediction_leaves_the_joint_missing(scene, value):
    def change(nxt, lut):
        r, c = scene["cells"][0, 7]
        nxt[2 * lut[7, 3] + 1, r, c] = value

    sc = _with_next(scene, change)
    items, got, gcand = _why(sc, scene["people"], scene["cand"])
    by = {(it["q"], it["j"]): it for it in items}
    assert by[0, 3]["why"] == "not finite" and by[0, 3]["support"] == 12
    assert gcand[0, 3] == -1 and (got[0, 3] == 0).all() and gcand[0, 9] == -2 and gcand[1, 5] == -2


def test_best_score_below_fill_threshold(scene):
    items, got, gcand = _why(scene, scene["people"], scene["cand"], fill_threshold=0.3126)
    assert all(it["why"] == "below fill_threshold" for it in items) and len(items) == 3
    assert np.array_equal(gcand, scene["cand"]) and np.array_equal(got, scene["people"])
    items, got, gcand = _why(scene, scene["people"], scene["cand"], fill_threshold=0.3125)  # >= : equality fills
    assert (gcand[scene["cand"] < 0] == -2).all()


def test_exclusion_of_other_peoples_peaks_and_the_own_dim_peak_two_cells_off(scene):
    """fill_radius 12 around person 0's joint 3 reaches person 1's held peak of joint 3 (0.75, the window's maximum): never taken.
    Person 0's own dim peak, moved two cells to the right of where its joints expect it, is."""
    sc = dict(scene, prob=scene["prob"].copy(), loc=scene["loc"].copy())
    r, c = scene["cells"][0, 3]
    r1, c1 = scene["cells"][1, 3]
    sc["prob"][3, r, c] = 0
    sc["prob"][3, r, c + 2] = 0.3125
    sc["loc"][6:8, r, c + 2] = scene["loc"][6:8, r, c]
    items, got, gcand = _why(sc, scene["people"], scene["cand"], fill_radius=12)
    it = [i for i in items if (i["q"], i["j"]) == (0, 3)][0]
    row0, col0 = int(it["e"][1] // 8), int(it["e"][0] // 8)
    assert (row0, col0) == (r, c)
    window = sc["prob"][3, max(row0 - 12, 0):row0 + 13, max(col0 - 12, 0):col0 + 13]
    assert abs(r1 - row0) <= 12 and abs(c1 - col0) <= 12 and window.max() == np.float32(0.75) == sc["prob"][3, r1, c1]
    assert it["cell"] == (r, c + 2) and gcand[0, 3] == -2 and got[0, 3, 2] == 0.3125
    assert np.abs(got[0, 3, :2] - (scene["joints"][0, 3] + (16.0, 0.0))).max() <= 1e-9
    # a dim value inside the other peak's NMS neighbourhood is excluded with it, even when it is all the window offers
    sc["prob"][3, r, c + 2] = 0
    sc["prob"][3, r1 + 1, c1 - 1] = 0.3125
    items, got, gcand = _why(sc, scene["people"], scene["cand"], fill_radius=12)
    assert gcand[0, 3] == -1
    sc["prob"][3, r1 + 2, c1 - 1] = 0.3125  # one cell further: free
    items, got, gcand = _why(sc, scene["people"], scene["cand"], fill_radius=12)
    assert gcand[0, 3] == -2 and [i for i in items if (i["q"], i["j"]) == (0, 3)][0]["cell"] == (r1 + 2, c1 - 1)


def test_ties_go_to_the_lower_cell_and_a_nan_score_is_never_chosen(scene):
    sc = dict(scene, prob=scene["prob"].copy())
    r, c = scene["cells"][0, 3]
    sc["prob"][3, r - 1, c + 1] = 0.3125  # an equal score at a lower row-major index
    sc["prob"][3, r + 1, c - 1] = 0.3125  # ... and at a higher one
    sc["prob"][3, r - 2, c - 2] = np.nan
    items, got, gcand = _why(sc, scene["people"], scene["cand"])
    assert [i for i in items if (i["q"], i["j"]) == (0, 3)][0]["cell"] == (r - 1, c + 1)
    assert not np.isnan(got).any()


# ---- the setting itself: no device needed ------------------------------------------------------------------------------------------
def _net():
    import caffe
    from deepcut_tools import deepercut_prototxt

    return caffe.Net(deepercut_prototxt(152, 64, 64), caffe.TEST, from_text=True)


BAD = [
    (dict(fill_threshold=0.0), "fill_threshold"),
    (dict(fill_threshold=-0.5), "fill_threshold"),
    (dict(fill_threshold=float("nan")), "fill_threshold"),
    (dict(fill_threshold=float("inf")), "fill_threshold"),
    (dict(fill_radius=-1), "fill_radius"),
    (dict(fill_radius=17), "fill_radius"),
    (dict(min_support=0), "min_support"),
]


def test_set_completion_in_python_without_a_device():
    import caffe

    net = _net()
    assert net.completion is None
    net.completion = True
    assert net.completion == caffe.pycaffe.COMPLETE_DEFAULTS and net.completion is not caffe.pycaffe.COMPLETE_DEFAULTS
    net.completion = dict(fill_threshold=0.375, fill_radius=16, min_support=3)
    assert net.completion == dict(fill_threshold=0.375, fill_radius=16, min_support=3)
    net.completion = dict(fill_radius=0)  # the others: the defaults
    assert net.completion == dict(caffe.pycaffe.COMPLETE_DEFAULTS, fill_radius=0)
    for kw, word in BAD:
        with pytest.raises(caffe.DeepcutError) as ei:
            net.completion = kw
        assert ei.value.code == -1 and word in str(ei.value), (kw, str(ei.value))
        assert net.completion == dict(caffe.pycaffe.COMPLETE_DEFAULTS, fill_radius=0)  # a refused value changes nothing
    with pytest.raises(ValueError) as ei:
        net.completion = dict(fill_treshold=0.3)
    assert "fill_treshold" in str(ei.value)
    with pytest.raises(TypeError):
        net.completion = 0.3
    # a clone has its net's setting at clone time, and one of its own afterwards
    c = net.clone()
    assert c.completion == net.completion
    net.completion = None
    assert net.completion is None and c.completion == dict(caffe.pycaffe.COMPLETE_DEFAULTS, fill_radius=0)
    assert net.clone().completion is None
    c.completion = False
    assert c.completion is None
    # a group has a setting of its own
    g = caffe.NetGroup([net, c])
    assert g.completion is None
    g.completion = dict(min_support=4)
    assert g.completion == dict(caffe.pycaffe.COMPLETE_DEFAULTS, min_support=4) and net.completion is None and c.completion is None
    for kw, word in BAD:
        with pytest.raises(caffe.DeepcutError) as ei:
            g.completion = kw
        assert ei.value.code == -1 and word in str(ei.value)
    g.completion = None
    assert g.completion is None


def test_a_complete_argument_is_refused_before_the_device_and_leaves_the_setting_alone():
    import caffe

    net = _net()
    net.completion = dict(fill_radius=5)
    before = net.completion
    edges = R.all_pairs_edges()
    with pytest.raises(caffe.DeepcutError) as ei:
        net.assemble_people(edges=edges, complete=dict(fill_radius=40))
    assert ei.value.code == -1 and "fill_radius" in str(ei.value)
    assert net.completion == before
    # a good one reaches the library's assembly entry, which has no CPU path; the net's own setting is back afterwards
    with pytest.raises(caffe.DeepcutError) as ei:
        net.assemble_people(edges=edges, complete=True)
    assert ei.value.code in (-5, -6) or "run forward() first" in str(ei.value)
    assert net.completion == before


def test_set_completion_through_the_c_abi_without_a_device():
    import caffe.pycaffe as pc

    L = pc._lib
    net = _net()
    good = dict(enabled=1, fill_threshold=0.25, fill_radius=2, min_support=2)
    out = pc.CompleteParams(9, 9.0, 9, 9)
    assert L.dc_net_get_completion(net._h, C.byref(out)) == 0
    assert (out.enabled, out.fill_threshold, out.fill_radius, out.min_support) == (0, 0.0, 0, 0)
    assert L.dc_net_set_completion(net._h, C.byref(pc.CompleteParams(**good))) == 0
    assert L.dc_net_get_completion(net._h, C.byref(out)) == 0
    assert (out.enabled, out.fill_threshold, out.fill_radius, out.min_support) == (1, 0.25, 2, 2)
    for kw, word in BAD:
        assert L.dc_net_set_completion(net._h, C.byref(pc.CompleteParams(**dict(good, **kw)))) == -1
        assert word.encode() in L.dc_last_error(), L.dc_last_error()
        assert L.dc_net_get_completion(net._h, C.byref(out)) == 0 and (out.enabled, out.fill_radius) == (1, 2)
    # not enabled: the other fields are not read
    assert L.dc_net_set_completion(net._h, C.byref(pc.CompleteParams(0, -1.0, 99, 0))) == 0
    assert L.dc_net_get_completion(net._h, C.byref(out)) == 0 and out.enabled == 0
    assert L.dc_net_set_completion(net._h, C.byref(pc.CompleteParams(**good))) == 0
    assert L.dc_net_set_completion(net._h, None) == 0  # NULL: off
    assert L.dc_net_get_completion(net._h, C.byref(out)) == 0 and out.enabled == 0
    assert L.dc_net_set_completion(None, None) == -1 and L.dc_net_get_completion(net._h, None) == -1
    # the group's entries
    import caffe

    g = caffe.NetGroup([net, net.clone()])
    assert L.dc_group_get_completion(g._h, C.byref(out)) == 0 and out.enabled == 0
    for kw, word in BAD:
        assert L.dc_group_set_completion(g._h, C.byref(pc.CompleteParams(**dict(good, **kw)))) == -1
        assert word.encode() in L.dc_last_error()
    assert L.dc_group_set_completion(g._h, C.byref(pc.CompleteParams(1, 0.5, 16, 1))) == 0
    assert L.dc_group_get_completion(g._h, C.byref(out)) == 0
    assert (out.enabled, out.fill_threshold, out.fill_radius, out.min_support) == (1, 0.5, 16, 1)
    assert L.dc_group_set_completion(g._h, None) == 0
    assert L.dc_group_get_completion(g._h, C.byref(out)) == 0 and out.enabled == 0

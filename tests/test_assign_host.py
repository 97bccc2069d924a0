"""CPU: step 4' of the tracking rule (include/deepcut_hip.h, dc_tracker_update) — the restatement in tests/assign_ref.py against
scipy.optimize.linear_sum_assignment, and the host side of the switch: dc_tracker_set_option / dc_tracker_get_option through ctypes and
`caffe.Tracker(assign=)` / `Tracker.assign`, without a device.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker; the rule pinned here is this project's own
definition, and an independent solver can only confirm the total it reaches, not the ties it breaks."""
import ctypes as C

import numpy as np
import pytest

import assign_ref as AR

EINVAL = -1  # include/deepcut_hip.h
OPT_ASSIGN, GREEDY, OPTIMAL = 1, 0, 1
GOOD = dict(slots=2, max_tracks=8, n_joints=14, max_misses=2, min_common=3, max_dist=0.5, min_size=16.0, motion=1)
INF = float("inf")


def _greedy(D, live, n, max_dist):
    """step 4 -> {place: person}"""
    pairs = sorted((float(D[i, q]), i, q) for i in range(len(live)) if live[i] for q in range(n) if D[i, q] <= max_dist)
    out, taken = {}, set()
    for _, i, q in pairs:
        if i not in out and q not in taken:
            out[i] = q
            taken.add(q)
    return out


def _case(rs, k):
    """A gated matrix with T, P <= 13: a fifth of the entries +inf, every third case quantised to quarters, some places not live"""
    T, P = int(rs.randint(1, 14)), int(rs.randint(1, 14))
    n = int(rs.randint(0, P + 1))
    D = rs.uniform(0.0, 3.0, (T, P))
    if k % 3 == 0:
        D = np.round(D * 4) / 4
    D[rs.rand(T, P) < 0.2] = INF
    D[:, n:] = INF
    live = [bool(x) for x in rs.rand(T) < 0.8]
    max_dist = 1.5 if k % 3 == 0 else float(rs.uniform(0.5, 2.5))
    return D, live, n, max_dist


def test_restatement_reaches_the_total_of_an_independent_solver():
    """300 seeded cases: the total of step 4' equals scipy's optimum within 1e-12, the matching is one-to-one over live places and the
    frame's people, every matched D <= max_dist, the total is never above greedy's, and greedy decides otherwise in some cases."""
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rs = np.random.RandomState(2024)
    differs, worst, below = 0, 0.0, 0
    for k in range(300):
        D, live, n, max_dist = _case(rs, k)
        pairs = AR.assign(D, live, n, max_dist)
        assert len(set(pairs.values())) == len(pairs) and all(live[i] and 0 <= q < n for i, q in pairs.items())
        assert all(D[i, q] <= max_dist for i, q in pairs.items())
        rows = [i for i in range(len(live)) if live[i]]
        got = AR.total(D, live, pairs, max_dist)
        if rows:
            cost = np.full((len(rows), n + len(rows)), max_dist, np.float64)
            gated = D[rows][:, :n]
            cost[:, :n] = np.where(gated <= max_dist, gated, INF)
            ri, ci = lsa(cost)
            want = float(cost[ri, ci].sum())
        else:
            want = 0.0
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-12, (k, got, want)
        g = _greedy(D, live, n, max_dist)
        gt = AR.total(D, live, g, max_dist)
        assert got <= gt + 1e-12, (k, got, gt)
        differs += g != pairs
        below += got < gt - 1e-9
    print("step 4' against linear_sum_assignment: max |total - optimum| = %.3e; greedy matched otherwise in %d of 300 cases and cost more "
          "in %d" % (worst, differs, below))
    assert differs >= 1 and below >= 1


def test_restatement_on_the_crossing_example_and_the_gate():
    """The example of the rule's text: D = [[2.25, 0.25], [12.25, 2.25]] at max_dist 16 — greedy takes 0.25 and is left with 12.25,
    step 4' keeps both identities for 4.5.  A pair at D == max_dist ties with a dummy column and the scan order gives it to the person
    (the real column comes first); a pair above max_dist, a NaN and a free place never match."""
    D = np.array([[2.25, 0.25], [12.25, 2.25]])
    assert _greedy(D, [True, True], 2, 16.0) == {0: 1, 1: 0}
    count = {}
    assert AR.assign(D, [True, True], 2, 16.0, count) == {0: 0, 1: 1} and count["trips"] >= 2
    assert AR.assign(np.array([[1.0]]), [True], 1, 1.0) == {0: 0}
    assert AR.assign(np.array([[np.nextafter(1.0, 2.0)]]), [True], 1, 1.0) == {}
    assert AR.assign(np.array([[float("nan")]]), [True], 1, 1.0) == {}
    assert AR.assign(np.array([[0.5], [0.25]]), [False, True], 1, 1.0) == {1: 0}
    assert AR.assign(np.array([[0.5, 0.25]]), [True], 1, 1.0) == {0: 0}  # person 1 is past the frame's people
    assert AR.assign(np.zeros((3, 0)), [True] * 3, 0, 1.0) == {} and AR.assign(np.zeros((2, 2)), [False] * 2, 2, 1.0) == {}


def _lib():
    import caffe.pycaffe as pc

    return pc, pc._lib


def test_option_round_trip_needs_no_device():
    pc, lib = _lib()
    q = pc.TrackerParams(GOOD["slots"], GOOD["max_tracks"], GOOD["n_joints"], None, GOOD["max_misses"], GOOD["min_common"], GOOD["max_dist"],
                         GOOD["min_size"], GOOD["motion"])
    h = C.c_void_p()
    assert lib.dc_tracker_create(C.byref(q), C.byref(h)) == 0 and h.value
    v = C.c_int(-7)
    assert lib.dc_tracker_get_option(h, OPT_ASSIGN, C.byref(v)) == 0 and v.value == GREEDY  # the default
    assert lib.dc_tracker_set_option(h, OPT_ASSIGN, OPTIMAL) == 0
    assert lib.dc_tracker_get_option(h, OPT_ASSIGN, C.byref(v)) == 0 and v.value == OPTIMAL
    assert lib.dc_tracker_set_option(h, 99, 0) == EINVAL and b"99" in lib.dc_last_error()
    assert lib.dc_tracker_get_option(h, 99, C.byref(v)) == EINVAL and b"99" in lib.dc_last_error()
    for bad in (2, -1):
        assert lib.dc_tracker_set_option(h, OPT_ASSIGN, bad) == EINVAL and str(bad).encode() in lib.dc_last_error()
    assert lib.dc_tracker_get_option(h, OPT_ASSIGN, C.byref(v)) == 0 and v.value == OPTIMAL  # a refused call changes nothing
    assert lib.dc_tracker_set_option(h, OPT_ASSIGN, GREEDY) == 0
    assert lib.dc_tracker_get_option(h, OPT_ASSIGN, C.byref(v)) == 0 and v.value == GREEDY
    assert lib.dc_tracker_set_option(None, OPT_ASSIGN, 0) == EINVAL and lib.dc_tracker_get_option(None, OPT_ASSIGN, C.byref(v)) == EINVAL
    assert lib.dc_tracker_get_option(h, OPT_ASSIGN, None) == EINVAL
    assert lib.dc_tracker_destroy(h) == 0


def test_python_assign_argument_and_property():
    import caffe

    _, lib = _lib()

    def c_value(t):
        v = C.c_int(-7)
        assert lib.dc_tracker_get_option(t._h, OPT_ASSIGN, C.byref(v)) == 0
        return v.value

    t = caffe.Tracker(**GOOD)
    assert t.assign == "greedy" and c_value(t) == GREEDY
    t.assign = "optimal"
    assert t.assign == "optimal" and c_value(t) == OPTIMAL
    assert lib.dc_tracker_set_option(t._h, OPT_ASSIGN, GREEDY) == 0 and t.assign == "greedy"  # the property reads the C value
    o = caffe.Tracker(assign="optimal", **GOOD)
    assert o.assign == "optimal" and c_value(o) == OPTIMAL and caffe.Tracker(assign="greedy", **GOOD).assign == "greedy"
    for bad in ("x", "", None, 1):
        with pytest.raises(ValueError) as ei:
            caffe.Tracker(assign=bad, **GOOD)
        assert "greedy" in str(ei.value) and "optimal" in str(ei.value)
        with pytest.raises(ValueError):
            o.assign = bad
    assert o.assign == "optimal"
    assert o.state(0)["ids"].tolist() == [-1] * 8  # still no device, nothing tracked


def test_pose_track_people_hands_assign_to_the_tracker_it_makes():
    """The generator refuses a bad `assign` when it makes its tracker, before any forward; a caller's tracker keeps its own setting."""
    from pose import track_people

    with pytest.raises(ValueError) as ei:
        next(track_people([np.zeros((8, 8, 3), np.uint8)], None, None, None, assign="x"))
    assert "greedy" in str(ei.value) and "optimal" in str(ei.value)

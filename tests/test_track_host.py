"""CPU: the host side of the tracker — every argument error of dc_tracker_* and of the chained dc_net_track_people /
dc_group_track_people, through ctypes and through `caffe.Tracker`, without a device; and self-checks of the restatement of the rule
(tests/track_ref.py).

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker; the rule pinned here is this project's own
definition (include/deepcut_hip.h, dc_tracker_update)."""
import ctypes as C

import numpy as np
import pytest

import people_ref as R
import track_ref as TR

EINVAL, ESHAPE, ENOCPU = -1, -3, -6  # include/deepcut_hip.h
GOOD = dict(slots=2, max_tracks=8, n_joints=14, sigma=None, max_misses=2, min_common=3, max_dist=0.5, min_size=16.0, motion=1)
BAD_CREATE = [
    (dict(slots=0), "slots"), (dict(slots=65), "slots"), (dict(max_tracks=0), "max_tracks"), (dict(max_tracks=257), "max_tracks"),
    (dict(n_joints=0), "n_joints"), (dict(n_joints=33), "n_joints"), (dict(sigma=[1.0] * 13 + [0.0]), "sigma of joint 13"),
    (dict(sigma=[1.0, float("nan")] + [1.0] * 12), "sigma of joint 1"), (dict(sigma=[float("inf")] + [1.0] * 13), "sigma of joint 0"),
    (dict(sigma=[-1.0] * 14), "sigma of joint 0"), (dict(max_misses=-1), "max_misses"), (dict(min_common=0), "min_common"),
    (dict(min_common=15), "min_common"), (dict(max_dist=-0.1), "max_dist"), (dict(max_dist=float("inf")), "max_dist"),
    (dict(max_dist=float("nan")), "max_dist"), (dict(min_size=0.0), "min_size"), (dict(min_size=float("inf")), "min_size"),
    (dict(min_size=float("nan")), "min_size"), (dict(motion=2), "motion"), (dict(motion=-1), "motion"),
]


def _lib():
    import caffe.pycaffe as pc

    return pc, pc._lib


def _create(**over):
    """dc_tracker_create through ctypes -> (return code, handle, message)"""
    pc, lib = _lib()
    a = dict(GOOD, **over)
    sig = None if a["sigma"] is None else np.ascontiguousarray(a["sigma"], np.float64)
    q = pc.TrackerParams(a["slots"], a["max_tracks"], a["n_joints"], None if sig is None else sig.ctypes.data, a["max_misses"], a["min_common"],
                         a["max_dist"], a["min_size"], a["motion"])
    h = C.c_void_p()
    rc = lib.dc_tracker_create(C.byref(q), C.byref(h))
    return rc, h, lib.dc_last_error().decode()


@pytest.mark.parametrize("over,names", BAD_CREATE, ids=["%s=%s" % (list(o)[0], str(list(o.values())[0])[:12]) for o, _ in BAD_CREATE])
def test_create_refuses_every_bad_parameter_by_name(over, names):
    import caffe

    rc, h, msg = _create(**over)
    assert rc == EINVAL and not h.value and names in msg, msg
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.Tracker(**dict(GOOD, **over))
    assert ei.value.code == EINVAL and names in str(ei.value)


def test_create_state_reset_and_destroy_need_no_device():
    import caffe

    _, lib = _lib()
    rc, h, msg = _create(sigma=[0.5] * 14, max_dist=0.0, max_misses=0, min_common=14, slots=64, max_tracks=256)  # the ends of the ranges
    assert rc == 0 and h.value, msg
    ids, misses, hits, poses = np.zeros(256, np.int64), np.ones(256, np.int32), np.ones(256, np.int32), np.ones((256, 14, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.dc_tracker_state(h, 63, vp(ids), vp(misses), vp(hits), vp(poses)) == 0
    assert (ids == -1).all() and not misses.any() and not hits.any() and not poses.any()  # before the first update every place is free
    assert lib.dc_tracker_state(h, 0, None, None, None, None) == 0
    for slot in (-1, 64):
        assert lib.dc_tracker_state(h, slot, vp(ids), None, None, None) == EINVAL and b"slot" in lib.dc_last_error()
    for slot in (-2, 64):
        assert lib.dc_tracker_reset(h, slot) == EINVAL and b"slot" in lib.dc_last_error()
    assert lib.dc_tracker_reset(h, -1) == 0 and lib.dc_tracker_reset(h, 63) == 0
    assert lib.dc_tracker_destroy(h) == 0 and lib.dc_tracker_destroy(None) == 0
    assert lib.dc_tracker_create(None, C.byref(C.c_void_p())) == EINVAL and lib.dc_tracker_state(None, 0, None, None, None, None) == EINVAL
    t = caffe.Tracker(**GOOD)
    st = t.state(1)
    assert st["ids"].tolist() == [-1] * 8 and st["poses"].shape == (8, 14, 3) and st["hits"].dtype == np.int32
    t.reset()
    t.reset(1)
    for call in (lambda: t.state(2), lambda: t.reset(2), lambda: t.reset(-2)):
        with pytest.raises(caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == EINVAL and "slot" in str(ei.value)
    with pytest.raises(ValueError):
        caffe.Tracker(n_joints=14, sigma=[1.0] * 13)


def test_update_checks_its_arguments_then_refuses_cpu_mode():
    import caffe

    _, lib = _lib()
    caffe.set_mode_cpu()
    t = caffe.Tracker(**GOOD)
    people = np.zeros((2, 4, 14, 3))
    ids = np.zeros((2, 4), np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def update(nb, P, n):
        n = np.ascontiguousarray(n, np.int32)
        return lib.dc_tracker_update(t._h, nb, P, vp(n), vp(people), vp(ids), None, None), lib.dc_last_error().decode()

    for nb in (0, 3, -1):
        rc, msg = update(nb, 4, [1, 1, 1])
        assert rc == EINVAL and "nb" in msg and "slots" in msg
    for P in (0, 257):
        rc, msg = update(2, P, [1, 1])
        assert rc == EINVAL and "max_people (P)" in msg
    for n in ([1, 5], [-1, 0]):
        rc, msg = update(2, 4, n)
        assert rc == EINVAL and "n_people[%d]" % (0 if n[0] < 0 else 1) in msg
    assert lib.dc_tracker_update(t._h, 1, 4, None, vp(people), vp(ids), None, None) == EINVAL
    assert lib.dc_tracker_update(t._h, 1, 4, vp(np.ones(1, np.int32)), None, vp(ids), None, None) == EINVAL
    assert lib.dc_tracker_update(t._h, 1, 4, vp(np.ones(1, np.int32)), vp(people), None, None, None) == EINVAL
    # good arguments: there is no CPU path
    rc, msg = update(2, 4, [4, 0])
    assert rc == ENOCPU and "CPU mode" in msg
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(people, [1, 2])
    assert ei.value.code == ENOCPU
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(np.zeros((3, 4, 14, 3)))  # three images, two slots
    assert ei.value.code == EINVAL
    with pytest.raises(ValueError):
        t.update(np.zeros((1, 4, 13, 3)))
    with pytest.raises(ValueError):
        t.update(people, [1])
    assert t.state(0)["ids"].tolist() == [-1] * 8  # nothing happened


def test_chained_entries_check_the_tracker_before_any_device_work():
    """nb <= slots, the tracker's joints against the net's, the assembly's own refusals first; then DC_ENOCPU."""
    import caffe
    from deepcut_tools import deepercut_prototxt

    caffe.set_mode_cpu()
    edges = R.all_pairs_edges()
    net2 = caffe.Net(deepercut_prototxt(152, 64, 64, 2), caffe.TEST, from_text=True)
    kw = dict(edges=edges, max_cost=20.0, seed_threshold=0.5)
    one_slot, two_slots, other_j = caffe.Tracker(n_joints=14, slots=1), caffe.Tracker(n_joints=14, slots=2), caffe.Tracker(n_joints=13, slots=2)
    grp = caffe.NetGroup([net2, net2.clone()])
    calls = {"net": lambda t, **k: net2.track_people(t, **dict(kw, **k)), "group": lambda t, **k: grp.track_people(t, [1.0, 0.5], 0, **dict(kw, **k))}
    for who, call in calls.items():
        with pytest.raises(caffe.DeepcutError) as ei:
            call(one_slot)
        assert ei.value.code == EINVAL and "slots" in str(ei.value), who
        with pytest.raises(caffe.DeepcutError) as ei:
            call(other_j)
        assert ei.value.code == ESHAPE and "13 joints" in str(ei.value), who
        with pytest.raises(caffe.DeepcutError) as ei:
            call(two_slots)
        assert ei.value.code == ENOCPU, who
        with pytest.raises(ValueError):  # the assembly's own checks are what they were
            call(two_slots, max_people=257)
        with pytest.raises(TypeError):
            call(None)
    # past the Python checks: max_people > 256 is the library's DC_EINVAL, a null tracker or a null ids array too
    pc, lib = _lib()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    e = np.ascontiguousarray(edges)
    count, people, ids = np.zeros(2, np.int32), np.zeros((2, 257, 14, 3)), np.zeros((2, 257), np.int64)
    q = pc.AssembleParams(1.0, 0.5, 1, 8, 20.0, 0.5, 257, 1)
    args = (C.byref(q), 182, vp(e), None, None, None, vp(count), vp(people), None, None)
    assert lib.dc_net_track_people(net2._h, two_slots._h, *args, vp(ids), None) == EINVAL and b"max_people" in lib.dc_last_error()
    q.max_people = 32
    assert lib.dc_net_track_people(net2._h, None, *args, vp(ids), None) == EINVAL and b"tracker" in lib.dc_last_error()
    assert lib.dc_net_track_people(net2._h, two_slots._h, *args, None, None) == EINVAL and b"ids" in lib.dc_last_error()
    assert lib.dc_net_track_people(net2._h, two_slots._h, *args, vp(ids), None) == ENOCPU
    sc = np.array([1.0, 0.5])
    assert lib.dc_group_track_people(grp._h, None, vp(sc), 0, None, *args, vp(ids), None) == EINVAL and b"tracker" in lib.dc_last_error()
    assert lib.dc_group_track_people(grp._h, two_slots._h, vp(sc), 0, None, *args, vp(ids), None) == ENOCPU
    # assemble_people is what it was
    with pytest.raises(caffe.DeepcutError) as ei:
        net2.assemble_people(**kw)
    assert ei.value.code == ENOCPU


# ---- self-checks of the restatement ---------------------------------------------------------------------------------------------
def _people(rs, n, J=6):
    out = np.zeros((n, J, 3), np.float64)
    for q in range(n):
        out[q, :, :2] = rs.uniform(50, 950, 2) + rs.uniform(-40, 40, (J, 2))
        out[q, :, 2] = rs.uniform(0.2, 1.0, J)
        out[q, rs.rand(J) < 0.2] = 0.0
    return out


@pytest.mark.parametrize("motion", [0, 1])
def test_restatement_permuting_a_frame_permutes_the_ids_and_nothing_else(motion):
    """A sequence without ties: the people of every frame in another order get the same ids, person by person, as long as births are
    not involved in the frame — a birth takes the next id in list order, which is the rule —, and the tracks end up the same."""
    J, T, P = 6, 12, 12
    rs = np.random.RandomState(7)
    prm = TR.params(J, rs.uniform(0.5, 2.0, J), max_misses=2, min_common=2, max_dist=0.05, min_size=10.0, motion=motion)
    world = _people(rs, 7)
    a, b = TR.Slot(T, J), TR.Slot(T, J)
    TR.update(a, world, 7, P, prm)
    TR.update(b, world, 7, P, prm)
    matched = 0
    for f in range(6):
        world = world.copy()
        world[:, :, :2] += rs.randn(7, J, 2) * 2.0 * (world[:, :, 2:] > 0)
        seen = np.sort(rs.permutation(7)[: 7 - (f % 3)])  # some are hidden in some frames, and come back
        perm = rs.permutation(len(seen))
        gaps = {}
        ids_a, place_a, D_a = TR.update(a, world[seen], len(seen), P, prm, gaps)
        ids_b, place_b, D_b = TR.update(b, world[seen][perm], len(seen), P, prm)
        assert gaps["choice"] > 1e-6  # no ties
        assert np.array_equal(ids_b[: len(seen)], ids_a[: len(seen)][perm]) and np.array_equal(place_b[: len(seen)], place_a[: len(seen)][perm])
        assert np.array_equal(D_b[:, : len(seen)], D_a[:, : len(seen)][:, perm])
        assert (ids_a[len(seen):] == -1).all() and (ids_b[len(seen):] == -1).all()
        for x, y in zip(TR.state(a), TR.state(b)):
            assert np.array_equal(x, y)
        matched += int((ids_a[: len(seen)] < 7).sum())
        assert sorted(ids_a[: len(seen)].tolist()) == sorted(seen.tolist())  # everybody keeps the id they were born with
    assert matched > 25 and a.next_id == 7


def test_restatement_motion_makes_no_difference_to_people_who_stand_still():
    J, T, P = 6, 8, 8
    rs = np.random.RandomState(2)
    world = _people(rs, 5)
    slots = {m: TR.Slot(T, J) for m in (0, 1)}
    prms = {m: TR.params(J, None, max_misses=1, min_common=2, max_dist=0.05, min_size=10.0, motion=m) for m in (0, 1)}
    for f in range(5):
        seen = [q for q in range(5) if (q + f) % 4]  # hidden now and then: misses + 1 multiplies a zero velocity
        out = {m: TR.update(slots[m], world[seen], len(seen), P, prms[m]) for m in (0, 1)}
        for x, y in zip(out[0], out[1]):
            assert np.array_equal(x, y)
        for x, y in zip(TR.state(slots[0]), TR.state(slots[1])):
            assert np.array_equal(x, y)
        assert not slots[1].vel.any()
    assert slots[0].next_id == 5 and max(slots[0].hits) >= 4


def test_restatement_by_hand():
    """Two tracks, hand-computed: the distance, the velocity after a miss, the prediction, the death and the reuse of a place."""
    prm = TR.params(2, [1.0, 2.0], max_misses=1, min_common=1, max_dist=1.0, min_size=4.0, motion=1)
    s = TR.Slot(2, 2)
    p0 = np.array([[(0, 0, 1), (8, 0, 1)], [(100, 100, 1), (0, 0, 0)]], np.float64)  # person 1 holds joint 0 only
    ids, place, D = TR.update(s, p0, 2, 2, prm)
    assert ids.tolist() == [0, 1] and np.isinf(D).all()
    # frame 2: person 0 moved by (2, 0); track 0 has size 8: D = ((4 / 64) + (4 / (64 * 4))) / 2; person 1 is not seen
    ids, place, D = TR.update(s, p0[:1] + np.array([2, 0, 0.0]), 1, 2, prm)
    assert D[0, 0] == (4 / 64.0 + 4 / 256.0) / 2 and D[1, 0] == (98.0 ** 2 + 100.0 ** 2) / 16.0 and ids.tolist() == [0, -1]
    assert s.vel[0].tolist() == [[2, 0], [2, 0]] and s.misses == [0, 1] and s.hits == [2, 1]
    # frame 3: the prediction (4, 0) / (12, 0) is met exactly: D = 0; track 1 misses a second time and dies; the newcomer takes its place
    ids, place, D = TR.update(s, np.stack([p0[1] + 50, (p0[0] + np.array([4, 0, 0.0]))]), 2, 2, prm)
    assert D[0, 1] == 0.0 and ids.tolist() == [2, 0] and place.tolist() == [1, 0] and s.next_id == 3

"""CPU: the host side of the tracker's step 8 (smoothed poses that bridge short gaps) — every argument error of
dc_tracker_set_smoothing through ctypes and through `caffe.Tracker`, without a device — and properties of the restatement of the rule
(tests/smooth_ref.py) alone: they show that the rule is worth having, and that the conditions the GPU tests hold the device to are
conditions the rule meets by itself.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker; the rule pinned here is this project's own
definition (include/deepcut_hip.h, dc_tracker_update, step 8)."""
import ctypes as C

import numpy as np
import pytest

import smooth_ref as SR
import smooth_scenes as SC
import track_ref as TR

EINVAL = -1  # include/deepcut_hip.h
GOOD = dict(enabled=1, min_cutoff=0.1, beta=4.0, d_cutoff=0.03, max_hold=3)
NAN, INF = float("nan"), float("inf")
BAD = [(dict(enabled=2), "enabled"), (dict(enabled=-1), "enabled"),
       (dict(min_cutoff=0.0), "min_cutoff"), (dict(min_cutoff=-0.1), "min_cutoff"), (dict(min_cutoff=NAN), "min_cutoff"),
       (dict(min_cutoff=INF), "min_cutoff"), (dict(beta=-1.0), "beta"), (dict(beta=NAN), "beta"), (dict(beta=INF), "beta"),
       (dict(d_cutoff=0.0), "d_cutoff"), (dict(d_cutoff=-1.0), "d_cutoff"), (dict(d_cutoff=NAN), "d_cutoff"), (dict(d_cutoff=INF), "d_cutoff"),
       (dict(max_hold=-1), "max_hold"), (dict(max_hold=1001), "max_hold")]


def _lib():
    import caffe.pycaffe as pc

    return pc, pc._lib


def _struct(pc, **over):
    a = dict(GOOD, **over)
    return pc.TrackSmoothParams(a["enabled"], a["min_cutoff"], a["beta"], a["d_cutoff"], a["max_hold"])


@pytest.mark.parametrize("over,name", BAD, ids=["%s=%s" % (list(o)[0], list(o.values())[0]) for o, _ in BAD])
def test_set_smoothing_refuses_every_bad_field_by_name(over, name):
    import caffe

    pc, lib = _lib()
    t = caffe.Tracker(n_joints=14)
    q = _struct(pc, **over)
    assert lib.dc_tracker_set_smoothing(t._h, C.byref(q)) == EINVAL
    assert name in lib.dc_last_error().decode(), lib.dc_last_error()
    assert t.smoothing is None  # a refused value changes nothing
    if "enabled" not in over:
        with pytest.raises(caffe.DeepcutError) as ei:
            t.smoothing = over
        assert ei.value.code == EINVAL and name in str(ei.value)
        with pytest.raises(caffe.DeepcutError) as ei:
            caffe.Tracker(n_joints=14, smooth=over)
        assert ei.value.code == EINVAL and name in str(ei.value)


def test_smoothing_round_trip_and_argument_handling():
    import caffe

    pc, lib = _lib()
    assert pc.SMOOTH_DEFAULTS == SR.PLACEHOLDERS == {"min_cutoff": 0.1, "beta": 4.0, "d_cutoff": 0.03, "max_hold": 3}
    t = caffe.Tracker(n_joints=14, slots=2, max_tracks=8)
    assert t.smoothing is None  # off by default
    for off in (None, False):
        t.smoothing = off
        assert t.smoothing is None
    t.smoothing = True
    assert t.smoothing == pc.SMOOTH_DEFAULTS
    t.smoothing = {"beta": 0.0, "max_hold": 0}  # the ends of the ranges; the rest are the defaults
    assert t.smoothing == dict(pc.SMOOTH_DEFAULTS, beta=0.0, max_hold=0)
    t.smoothing = {"max_hold": 1000, "min_cutoff": 1.0 / 30.0}
    assert t.smoothing == dict(pc.SMOOTH_DEFAULTS, max_hold=1000, min_cutoff=1.0 / 30.0)
    t.smoothing = None
    assert t.smoothing is None
    assert caffe.Tracker(n_joints=14, smooth=True).smoothing == pc.SMOOTH_DEFAULTS
    assert caffe.Tracker(n_joints=14, smooth={"d_cutoff": 0.5}).smoothing == dict(pc.SMOOTH_DEFAULTS, d_cutoff=0.5)
    assert caffe.Tracker(n_joints=14, smooth=False).smoothing is None and caffe.Tracker(n_joints=14).smoothing is None
    with pytest.raises(TypeError):
        caffe.Tracker(n_joints=14, smooth=3)
    with pytest.raises(ValueError) as ei:
        caffe.Tracker(n_joints=14, smooth={"cutoff": 1.0})
    assert "cutoff" in str(ei.value)
    with pytest.raises(ValueError):
        t.smoothing = {"max_hold": "many"}
    # the C entries: NULL and enabled == 0 are off; get wants somewhere to write; no device was needed for any of this
    q = _struct(pc)
    assert lib.dc_tracker_set_smoothing(t._h, C.byref(q)) == 0 and t.smoothing == pc.SMOOTH_DEFAULTS
    q = _struct(pc, enabled=0, min_cutoff=NAN)  # the fields of a switched-off struct are not looked at
    assert lib.dc_tracker_set_smoothing(t._h, C.byref(q)) == 0 and t.smoothing is None
    assert lib.dc_tracker_set_smoothing(None, None) == EINVAL and lib.dc_tracker_get_smoothing(t._h, None) == EINVAL
    # before the first update every filter is empty
    t.smoothing = True
    st = t.smooth_state(1)
    assert st["poses"].shape == (8, 14, 3) and not st["poses"].any() and st["gap"].dtype == np.int32 and (st["gap"] == -1).all()
    with pytest.raises(caffe.DeepcutError) as ei:
        t.smooth_state(2)
    assert ei.value.code == EINVAL and "slot" in str(ei.value)
    t.reset()
    t.reset(1)


def test_update_smoothed_is_refused_with_smoothing_off():
    import caffe

    _, lib = _lib()
    t = caffe.Tracker(n_joints=14, slots=1, max_tracks=4)
    people = np.zeros((1, 2, 14, 3))
    with pytest.raises(caffe.DeepcutError) as ei:
        t.update(people, [1], return_smooth=True)
    assert ei.value.code == EINVAL and "smoothing is off" in str(ei.value)
    n, ids = np.ones(1, np.int32), np.zeros((1, 2), np.int64)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert lib.dc_tracker_update_smoothed(t._h, 1, 2, None, vp(n), vp(people), vp(ids), None, None, None, None) == EINVAL
    assert b"smoothing" in lib.dc_last_error()


# ---- the restatement alone ----------------------------------------------------------------------------------------------------
def _run(raw, prm, hide=None, cases=None):
    """One walker through the restated rule.  raw: [frames, J, 3]; hide = (joint, first frame, count): that joint is (0, 0, 0) then.
    -> (smooth [frames, J, 3], src [frames, J], the Tracked object)."""
    tr = SR.Tracked(TR, 4, SC.J, TR.params(SC.J, None, **SC.TRACK), prm)
    smooth, src = [], []
    for f in range(len(raw)):
        pose = raw[f].copy()
        if hide is not None and hide[1] <= f < hide[1] + hide[2]:
            pose[hide[0]] = 0.0
        ids, place, s, r = tr.update(pose[None], 1, 2, cases)
        assert ids[0] == 0 and place[0] == 0, f  # one track throughout
        assert not s[1].any() and not r[1].any()
        smooth.append(s[0])
        src.append(r[0])
    return np.array(smooth), np.array(src), tr


def test_exact_walker_is_returned_exactly():
    """A rigid figure translating by (3.0, 1.5) pixels a frame, every coordinate dyadic: prediction and observation coincide, so the
    smoothed poses ARE the raw ones; likewise a figure that stands still."""
    prm = SR.params(**SR.PLACEHOLDERS)
    for v in ((3.0, 1.5), (0.0, 0.0)):
        raw = SC.walker(24, *v)
        cases = {}
        smooth, src, _ = _run(raw, prm, cases=cases)
        assert np.array_equal(smooth, raw) and (src == 1).all()
        assert cases["8a_first"] == SC.J and cases["8a_second"] == SC.J and cases["8a_running"] == 22 * SC.J


def test_exact_walker_bridges_a_short_gap_on_the_true_position():
    prm = SR.params(**dict(SR.PLACEHOLDERS, max_hold=3))
    raw = SC.walker(24, 3.0, 1.5)
    smooth, src, tr = _run(raw, prm, hide=(5, 10, 2))
    assert src[10:12, 5].tolist() == [2, 2] and (np.delete(src, 5, axis=1) == 1).all() and (src[:10, 5] == 1).all() and (src[12:, 5] == 1).all()
    assert np.array_equal(smooth, raw)  # the bridged joint sits exactly on the true position, with the last observed score
    assert tr.filt.n[0][5] == 2


def test_exact_walker_gives_up_after_max_hold_and_starts_again():
    prm = SR.params(**dict(SR.PLACEHOLDERS, max_hold=3))
    raw = SC.walker(24, 3.0, 1.5)
    cases = {}
    smooth, src, tr = _run(raw[:15], prm, hide=(5, 10, 4), cases=cases)
    assert src[10:14, 5].tolist() == [2, 2, 2, 0] and np.array_equal(smooth[10:13], raw[10:13]) and not smooth[13, 5].any()
    assert cases["8a_bridged"] == 3 and cases["8a_expired"] == 1
    assert src[14, 5] == 1 and np.array_equal(smooth[14], raw[14]) and tr.filt.n[0][5] == 1  # it starts again: one observation
    assert all(tr.filt.n[0][j] == 2 for j in range(SC.J) if j != 5)


@pytest.mark.parametrize("seed", range(8))
def test_noisy_walker_is_smoother_and_closer_to_the_truth(seed):
    """The figure at 0, 3 and 12 pixels a frame with N(0, 1.5 px) noise per joint and frame, 120 frames, the placeholder parameters.
    After 40 frames: the RMS second difference of the smoothed joints is <= 0.5 x the raw one, and the mean absolute error against the
    true positions <= 0.9 x the raw one."""
    prm = SR.params(**SR.PLACEHOLDERS)
    for v in SC.SPEEDS:
        truth = SC.walker(120, v, 0.5 * v)
        raw = SC.noisy(truth, seed)
        smooth, src, _ = _run(raw, prm)
        assert (src == 1).all()
        jerk, err = SC.ratios(truth, raw, smooth)
        print("noisy walker, seed %d, %g px/frame: second difference %.3f x raw, error %.3f x raw" % (seed, v, jerk, err))
        assert jerk <= 0.5 and err <= 0.9

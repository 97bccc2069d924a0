"""-m gpu: step 8 of the tracker's rule — smoothed poses that bridge short gaps (dc_tracker_set_smoothing, dc_tracker_update_smoothed,
dc_tracker_smooth_state and the chained entries; csrc/track.hip) — against the float64 restatement in tests/smooth_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker.  The rule is this project's own
(include/deepcut_hip.h, dc_tracker_update, step 8); what is proven here is that the device computes what the restatement computes: src,
gap and which joints are bridged exactly — they depend on held flags and integer counters only —, the smoothed poses and the filters'
expectations within 1e-9 * max(1, |value|), the bound the tracker's distances are held to (it covers fused multiply-adds); and that
smoothing changes no decision: ids, place, dist and the slots' state are bit for bit those of a tracker without it."""
import numpy as np
import pytest

import assign_ref as AR
import people_ref as R
import smooth_ref as SR
import smooth_scenes as SC
import track_ref as TR

pytestmark = pytest.mark.gpu

J = 14
RULES = {"greedy": TR.associate, "optimal": AR.associate}
TOL = 1e-9


def _random_people(rs, n, joints=J, lo=0.0, hi=500.0, p_missing=0.25):
    """n people of `joints` joints around random centres: x, y, score; a missing joint is (0, 0, 0)."""
    out = np.zeros((n, joints, 3), np.float64)
    for q in range(n):
        c = rs.uniform(lo + 60, hi - 60, 2)
        out[q, :, :2] = c + rs.uniform(-50, 50, (joints, 2))
        out[q, :, 2] = rs.uniform(0.1, 1.0, joints)
        out[q, rs.rand(joints) < p_missing] = 0.0
    return out


def _jitter(rs, people, sd, p_flip=0.1):
    """The same people a frame later: every held joint moved by N(0, sd), a few joints appearing / vanishing (they flicker)."""
    out = people.copy()
    held = out[:, :, 2] > 0
    out[:, :, :2] += rs.randn(*out[:, :, :2].shape) * sd * held[:, :, None]
    flip = rs.rand(*held.shape) < p_flip
    for q, j in zip(*np.nonzero(flip)):
        if held[q, j]:
            out[q, j] = 0.0
        else:
            out[q, j] = (out[q, held[q], 0].mean() if held[q].any() else 100.0, out[q, held[q], 1].mean() if held[q].any() else 100.0, 0.5)
    return out


def _pack(frames, P):
    """a list of [m_b, J, 3] -> (people [nb, P, J, 3], n [nb])"""
    ppl = np.zeros((len(frames), P, frames[0].shape[1], 3), np.float64)
    for b, f in enumerate(frames):
        ppl[b, :len(f)] = f
    return ppl, np.array([len(f) for f in frames], np.int32)


def _sequence(seed, P, updates=12, start=(12, 19)):
    """Per update the frames of two slots, built as test_gpu_track.py builds its random sequence: people jitter, vanish for good,
    appear, are hidden for a frame or two, change order, and joints flicker.  Slot 1 grows past the 20 track places."""
    rs = np.random.RandomState(seed)
    world = [_random_people(rs, k) for k in start]
    hide = [np.zeros(k, np.int64) for k in start]  # frames a person stays hidden, this one included
    out = []
    for u in range(updates):
        frames = []
        for b in range(2):
            w = _jitter(rs, world[b], 3.0, p_flip=0.15)
            keep = rs.rand(len(w)) > 0.08  # people vanish for good ...
            w, h = w[keep], hide[b][keep]
            if rs.rand() < 0.7 and len(w) < P:  # ... and appear
                w = np.concatenate([w, _random_people(rs, 1 + int(rs.rand() < 0.5 and len(w) + 1 < P))])
                h = np.concatenate([h, np.zeros(len(w) - len(h), np.int64)])
            h = np.where(h > 0, h, (rs.rand(len(w)) < 0.2) * rs.randint(1, 4, len(w)))  # and some are missed for one to three frames
            frames.append(w[h == 0][rs.permutation(int((h == 0).sum()))])  # in any order
            world[b], hide[b] = w, np.maximum(h - 1, 0)
        out.append(frames)
    return out


def _close(got, want):
    """max |got - want| / max(1, |want|)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want) / np.maximum(1.0, np.abs(want))).max()) if got.size else 0.0


class _Both(object):
    """A tracker with smoothing on the device and the restatement beside it: steps 4-7 restated on the DEVICE's own distances (as the
    tracker's own tests do), step 8 restated behind them."""

    def __init__(self, caffe, S, T, joints, tkw, skw, assign="greedy", sigma=None):
        self.tracker = caffe.Tracker(n_joints=joints, slots=S, max_tracks=T, sigma=sigma, assign=assign, smooth=skw, **tkw)
        self.tprm, self.sprm = TR.params(joints, sigma, **tkw), SR.params(**skw)
        self.slots = [TR.Slot(T, joints) for _ in range(S)]
        self.filts = [SR.Filters(T, joints) for _ in range(S)]
        self.rule, self.cases, self.worst, self.bridged = RULES[assign], {}, 0.0, 0

    def step(self, frames, P, slot_of=None):
        ppl, n = _pack(frames, P)
        ids, place, dist, smooth, src = self.tracker.update(ppl, n, return_dist=True, slot_of=slot_of, return_smooth=True)
        assert smooth.shape == ppl.shape and src.shape == ppl.shape[:3] and src.dtype == np.int32
        for b in range(len(frames)):
            k = b if slot_of is None else slot_of[b]
            before = SR.snapshot(self.slots[k])
            rid, rplace = self.rule(self.slots[k], dist[b], ppl[b], int(n[b]), P, self.tprm)
            assert np.array_equal(ids[b], rid) and np.array_equal(place[b], rplace), b
            want, wsrc = SR.step8(self.filts[k], before, self.slots[k], ppl[b], int(n[b]), P, rid, rplace, self.tprm["min_size"], self.sprm,
                                  self.cases)
            assert np.array_equal(src[b], wsrc), b  # exact: held flags and integer counters only
            assert not smooth[b][src[b] == 0].any()
            self.worst = max(self.worst, _close(smooth[b], want))
            self.bridged += int((src[b] == 2).sum())
        for k in set(range(len(frames)) if slot_of is None else slot_of):
            st = self.tracker.smooth_state(k)
            wposes, wgap = SR.state(self.filts[k])
            assert np.array_equal(st["gap"], wgap), k  # exact
            self.worst = max(self.worst, _close(st["poses"], wposes))
        return ids, place, dist, smooth, src


SEQ_T, SEQ_P = 20, 24
SEQ_TKW = dict(max_misses=3, min_common=3, max_dist=0.03, min_size=20.0)
SEQ_SKW = dict(min_cutoff=0.1, beta=4.0, d_cutoff=0.03, max_hold=2)


@pytest.mark.parametrize("motion", [0, 1])
@pytest.mark.parametrize("assign", ["greedy", "optimal"])
def test_device_equals_the_restatement_on_a_random_sequence(gpu_caffe, assign, motion):
    """S = 2, T = 20, P = 24, J = 14 (T * J and P * J above 256: the strided loops of step 8 take a second trip), 12 updates in which
    people vanish, appear, are hidden for a frame and joints flicker; a random sigma.  Every case of 8a, 8b and 8c occurs."""
    sigma = np.random.RandomState(21).uniform(0.5, 2.0, J)
    both = _Both(gpu_caffe, 2, SEQ_T, J, dict(SEQ_TKW, motion=motion), SEQ_SKW, assign, sigma)
    for frames in _sequence(7, SEQ_P):
        both.step(frames, SEQ_P)
    print("smoothing, %s, motion %d: cases %r; %d bridged joints; max |device - restatement| / max(1, |value|) = %.3e"
          % (assign, motion, both.cases, both.bridged, both.worst))
    missing = [c for c in SR.CASES if both.cases.get(c, 0) < 1]
    assert not missing, missing
    assert both.bridged > 0 and both.worst <= TOL


def _run_plain(caffe, frames_per_update, smooth, assign="greedy"):
    """The sequence on a tracker with or without smoothing -> per update (ids, place, dist, the slots' state[, smooth, src])."""
    tracker = caffe.Tracker(n_joints=J, slots=2, max_tracks=SEQ_T, assign=assign, smooth=smooth, motion=1, **SEQ_TKW)
    log = []
    for frames in frames_per_update:
        ppl, n = _pack(frames, SEQ_P)
        out = tracker.update(ppl, n, return_dist=True, return_smooth=smooth is not None)
        log.append(tuple(out[:3]) + ([tracker.state(b) for b in range(2)],) + tuple(out[3:]))
    return log


@pytest.mark.parametrize("assign", ["greedy", "optimal"])
def test_smoothing_changes_no_decision_and_is_deterministic(gpu_caffe, assign):
    """The same sequence on a tracker without smoothing and on two with it: ids, place, dist and state() are bit for bit equal in all
    three, and the two smoothed runs agree on smooth and src bit for bit."""
    seq = _sequence(7, SEQ_P)
    off, on, again = [_run_plain(gpu_caffe, seq, s, assign) for s in (None, SEQ_SKW, SEQ_SKW)]
    differs = 0
    for u, (a, b, c) in enumerate(zip(off, on, again)):
        for other in (b, c):
            assert all(np.array_equal(a[k], other[k]) for k in range(3)), u
            assert all(np.array_equal(x[key], y[key]) for x, y in zip(a[3], other[3]) for key in x), u
        assert np.array_equal(b[4], c[4]) and np.array_equal(b[5], c[5]), u
        ppl, _ = _pack(seq[u], SEQ_P)
        differs += int((b[4] != ppl).any())
    assert differs >= 8  # the smoothed poses are not the raw ones


def test_slot_map_equals_one_image_per_call(gpu_caffe):
    """8 frames of slot 1 in one call against eight calls: ids, place, dist, smooth, src, the state and the filters, bit for bit."""
    frames = [f[1] for f in _sequence(7, SEQ_P)[:8]]
    kw = dict(n_joints=J, slots=2, max_tracks=SEQ_T, smooth=SEQ_SKW, motion=1, **SEQ_TKW)
    one, many = gpu_caffe.Tracker(**kw), gpu_caffe.Tracker(**kw)
    ppl, n = _pack(frames, SEQ_P)
    got = one.update(ppl, n, return_dist=True, slot_of=[1] * 8, return_smooth=True)
    for b in range(8):
        want = many.update(ppl[b:b + 1], n[b:b + 1], return_dist=True, slot_of=[1], return_smooth=True)
        assert all(np.array_equal(g[b], w[0]) for g, w in zip(got, want)), b
    assert (got[4] == 2).any() and (got[0] >= 0).any()
    for k in (0, 1):
        a, b = one.smooth_state(k), many.smooth_state(k)
        assert all(np.array_equal(a[key], b[key]) for key in a)
        a, b = one.state(k), many.state(k)
        assert all(np.array_equal(a[key], b[key]) for key in a)
    assert (one.smooth_state(0)["gap"] == -1).all() and (one.smooth_state(1)["gap"] >= 0).any()  # the slot no image named is untouched


def test_full_size_equals_the_restatement(gpu_caffe):
    """T = P = n = 256, J = 32 once (256 x 32 items of either kind): three updates of people on a 100-pixel grid — born, then jittered
    and reordered with flickering joints and a few people hidden, then all back."""
    T = P = 256
    joints = 32
    rs = np.random.RandomState(13)
    centres = np.array([(100.0 * (k % 16) + 50, 100.0 * (k // 16) + 50) for k in range(256)])
    first = np.zeros((256, joints, 3))
    first[:, :, :2] = centres[:, None, :] + rs.uniform(-20, 20, (256, joints, 2))
    first[:, :, 2] = rs.uniform(0.2, 1.0, (256, joints))
    second = _jitter(rs, first, 1.0, p_flip=0.1)
    third = _jitter(rs, second, 1.0, p_flip=0.1)
    hidden = rs.rand(256) < 0.1
    both = _Both(gpu_caffe, 1, T, joints, dict(max_misses=1, min_common=2, max_dist=0.5, min_size=20.0, motion=1), dict(SEQ_SKW, max_hold=1))
    ids, _, _, smooth, src = both.step([first], P)
    assert ids[0].tolist() == list(range(256)) and np.array_equal(smooth[0], first) and (src[0] == 1).all()
    both.step([second[~hidden][rs.permutation(int((~hidden).sum()))]], P)
    ids, _, _, _, src = both.step([third[rs.permutation(256)]], P)
    print("smoothing at full size: cases %r, max |device - restatement| / max(1, |value|) = %.3e" % (both.cases, both.worst))
    assert sorted(ids[0].tolist()) == list(range(256)) and (src[0] == 2).any()
    assert all(both.cases.get(c, 0) > 0 for c in ("8a_running", "8a_bridged", "8b_aged", "8a_second")) and both.worst <= TOL


# ---- the walkers of the host test, on the device ----------------------------------------------------------------------------------
def _walk_on_device(caffe, raw, skw, hide=None):
    """One walker through a tracker with smoothing, up to 60 frames a call -> (smooth [frames, J, 3], src [frames, J], tracker)."""
    tracker = caffe.Tracker(n_joints=SC.J, slots=1, max_tracks=4, smooth=skw, **SC.TRACK)
    poses = raw.copy()
    if hide is not None:
        poses[hide[1]:hide[1] + hide[2], hide[0]] = 0.0
    smooth, src = [], []
    for at in range(0, len(poses), 60):
        part = poses[at:at + 60]
        ids, place, s, r = tracker.update(part[:, None], np.ones(len(part), np.int32), slot_of=[0] * len(part), return_smooth=True)
        assert (ids[:, 0] == 0).all() and (place[:, 0] == 0).all()
        smooth.append(s[:, 0])
        src.append(r[:, 0])
    return np.concatenate(smooth), np.concatenate(src), tracker


def test_exact_walker_on_the_device(gpu_caffe):
    """The rigid figure at (3.0, 1.5) pixels a frame, and standing still, every coordinate dyadic: smoothed == raw exactly; a joint removed
    for 2 frames at max_hold = 3 is bridged exactly on the true position; removed for 4, the fourth frame gives src 0 and the joint starts
    again when it returns."""
    skw = dict(SR.PLACEHOLDERS, max_hold=3)
    for v in ((3.0, 1.5), (0.0, 0.0)):
        raw = SC.walker(24, *v)
        smooth, src, _ = _walk_on_device(gpu_caffe, raw, skw)
        assert np.array_equal(smooth, raw) and (src == 1).all()
    raw = SC.walker(24, 3.0, 1.5)
    smooth, src, _ = _walk_on_device(gpu_caffe, raw, skw, hide=(5, 10, 2))
    assert src[10:12, 5].tolist() == [2, 2] and (src == 2).sum() == 2 and (src > 0).all()
    assert np.array_equal(smooth, raw)
    smooth, src, tracker = _walk_on_device(gpu_caffe, raw[:15], skw, hide=(5, 10, 4))
    assert src[10:14, 5].tolist() == [2, 2, 2, 0] and np.array_equal(smooth[10:13], raw[10:13]) and not smooth[13, 5].any()
    assert src[14, 5] == 1 and np.array_equal(smooth[14], raw[14])
    st = tracker.smooth_state()
    assert (st["gap"][0] == 0).all() and np.array_equal(st["poses"][0, 5], raw[14, 5])  # one observation: it is expected where it was seen
    assert np.array_equal(np.delete(st["poses"][0], 5, axis=0), np.delete(raw[14], 5, axis=0))


@pytest.mark.parametrize("seed", range(4))
def test_noisy_walker_on_the_device(gpu_caffe, seed):
    """The conditions of the host test, met by the device: after 40 of 120 frames the RMS second difference of the smoothed joints is
    <= 0.5 x the raw one and the mean absolute error against the truth <= 0.9 x the raw one, at 0, 3 and 12 pixels a frame, N(0, 1.5 px)
    noise, the placeholder parameters."""
    for v in SC.SPEEDS:
        truth = SC.walker(120, v, 0.5 * v)
        raw = SC.noisy(truth, seed)
        smooth, src, _ = _walk_on_device(gpu_caffe, raw, dict(SR.PLACEHOLDERS))
        assert (src == 1).all()
        jerk, err = SC.ratios(truth, raw, smooth)
        print("noisy walker on the device, seed %d, %g px/frame: second difference %.3f x raw, error %.3f x raw" % (seed, v, jerk, err))
        assert jerk <= 0.5 and err <= 0.9


def test_set_smoothing_between_updates(gpu_caffe):
    """Off -> on starts with empty filters; a parameter change while on keeps them; reset(slot) clears the slot's."""
    tkw, skw = dict(SC.TRACK), dict(SR.PLACEHOLDERS)
    raw = SC.noisy(SC.walker(12, 3.0, 1.5), 5)
    tracker = gpu_caffe.Tracker(n_joints=SC.J, slots=2, max_tracks=4, smooth=skw, **tkw)
    ref = [SR.Tracked(TR, 4, SC.J, TR.params(SC.J, None, **tkw), SR.params(**skw)) for _ in range(2)]

    def step(f, smoothed=True):
        ppl = np.stack([raw[f][None], raw[f][None] + (500.0, 0.0, 0.0)])  # the same walker in both slots, slot 1's 500 pixels to the right
        out = tracker.update(ppl, [1, 1], return_smooth=smoothed)
        worst = 0.0
        for b in range(2):
            ids, place, want, wsrc = ref[b].update(ppl[b], 1, 1)
            assert out[0][b, 0] == ids[0] == 0
            if smoothed:
                assert np.array_equal(out[3][b], wsrc)
                worst = max(worst, _close(out[2][b], want))
        assert worst <= TOL
        return out

    for f in range(4):
        step(f)
    running = tracker.smooth_state(0)
    assert (running["gap"][0] == 0).all() and (running["gap"][1:] == -1).all()
    # a parameter change while on keeps the filters, and the next update uses the new value
    changed = dict(skw, beta=0.5, min_cutoff=0.02)
    tracker.smoothing = changed
    assert tracker.smoothing == changed
    kept = tracker.smooth_state(0)
    assert all(np.array_equal(running[k], kept[k]) for k in running)
    for r in ref:
        r.prm = SR.params(**changed)
    out = step(4)
    assert (out[2][0, 0] != raw[4]).any()  # a running filter: smoothed, not raw
    # reset(0) clears slot 0's filters with its tracks and leaves slot 1's
    tracker.reset(0)
    ref[0] = SR.Tracked(TR, 4, SC.J, ref[0].tprm, ref[0].prm)
    assert (tracker.smooth_state(0)["gap"] == -1).all() and not tracker.smooth_state(0)["poses"].any()
    assert (tracker.smooth_state(1)["gap"][0] == 0).all()
    out = step(5)
    assert np.array_equal(out[2][0, 0], raw[5])  # slot 0 starts again: the first observation comes back as given
    # off: the plain update goes on tracking; back on, every filter is empty although the tracks live on
    tracker.smoothing = None
    assert (tracker.smooth_state(1)["gap"] == -1).all()
    with pytest.raises(gpu_caffe.DeepcutError):
        tracker.update(np.stack([raw[6][None]] * 2), [1, 1], return_smooth=True)
    step(6, smoothed=False)
    tracker.smoothing = skw
    assert all((tracker.smooth_state(k)["gap"] == -1).all() for k in (0, 1))
    for b in range(2):
        ref[b].filt.reset()
        ref[b].prm = SR.params(**skw)
    out = step(7)
    assert np.array_equal(out[2][1, 0], raw[7] + (500.0, 0.0, 0.0)) and tracker.state(1)["hits"][0] == 8
    step(8)
    step(9)


# ---- chained entries ----------------------------------------------------------------------------------------------------------
H, W = 200, 264
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))
EDGES = R.all_pairs_edges()
AKW = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
SKW = dict(SR.PLACEHOLDERS)
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(4)]
CHAIN = dict(edges=EDGES, mean=MEAN, std=STD, **AKW)
STAGES = [dict(), dict(complete=True, dedupe=True)]
STAGE_IDS = ["plain", "complete_dedupe"]
_nets = {}


@pytest.fixture(scope="module", autouse=True)
def cost_model_tiles():
    """DC_AUTOTUNE=0 for every forward of the module: the tiles are the cost model's, nothing is timed."""
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
    from deepcut_tools import deepercut_prototxt

    if kind not in _nets:
        kw = {"f32": dict(), "sparse": dict(want=["loc_pred", "prob"], sparse_pairwise=True)}[kind]
        _nets[kind] = caffe.Net(deepercut_prototxt(152, H, W), path, caffe.TEST, from_text=True, **kw)
    return _nets[kind]


def _plant(people):
    """The first (person, joint) the assembly left not held, and the joint to plant there: the mean of the person's held joints."""
    for q in range(len(people)):
        held = people[q, :, 2] > 0
        if held.any() and not held.all():
            j = int(np.nonzero(~held)[0][0])
            return q, j, (float(people[q, held, 0].mean()), float(people[q, held, 1].mean()), 0.5)
    raise AssertionError("the scene has no person with a joint missing: nothing to bridge")


def _seeded(caffe, people, smooth):
    """A tracker that has seen the frame's own people twice, moved a little, one of them with an extra planted joint: at the next update
    with these people every held joint's filter is running, and the planted joint is bridged."""
    tracker = caffe.Tracker(n_joints=J, smooth=smooth, **TKW)
    q, j, joint = _plant(people)
    for shift in ((-4.0, -2.0), (-1.5, 0.5)):
        seed = people.copy()
        seed[q, j] = joint
        seed[:, :, :2] += np.array(shift) * (seed[:, :, 2:3] > 0)
        ids, _ = tracker.update([seed])
        assert ids[0, :len(people)].tolist() == list(range(len(people)))
    return tracker, q, j


def _check_entry(caffe, want, entry):
    """want: assemble_people's dict of the frame; entry(tracker) -> the chained entry's dict of it.  With smoothing on people and bridged
    are what a second, identically seeded tracker's update(..., return_smooth=True) returns on assemble_people's people, bit for bit; cand
    is the assembly's except -3 at the bridged joint; ids are those of a tracker without smoothing, whose call returns the assembly's
    people bit for bit."""
    people, m = want["people"], len(want["people"])
    assert m > 0
    on, q, j = _seeded(caffe, people, SKW)
    by_hand, _, _ = _seeded(caffe, people, SKW)
    off, _, _ = _seeded(caffe, people, None)
    got, raw = entry(on), entry(off)
    ids, place, smooth, src = by_hand.update([people], return_smooth=True)
    assert "bridged" not in raw and np.array_equal(raw["people"], people) and np.array_equal(raw["cand"], want["cand"])
    assert np.array_equal(got["people"], smooth[0, :m]) and np.array_equal(got["bridged"], src[0, :m] == 2)
    assert got["bridged"][q, j] and got["bridged"].sum() == 1 and got["people"][q, j, 2] == 0.5
    assert (got["people"] != people).sum() > 3  # running filters: smoothed, not raw
    cand = want["cand"].copy()
    assert cand[q, j] == -1
    cand[q, j] = -3
    assert np.array_equal(got["cand"], cand)
    assert np.array_equal(got["ids"], raw["ids"]) and np.array_equal(got["place"], raw["place"]) and np.array_equal(got["ids"], ids[0, :m])
    a, b = on.state(), off.state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    a, b = on.smooth_state(), by_hand.smooth_state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    if "filled" in want:
        assert np.array_equal(got["filled"], want["filled"])
    return m


@pytest.mark.parametrize("stages", STAGES, ids=STAGE_IDS)
@pytest.mark.parametrize("kind", ["f32", "sparse"])
def test_net_track_people_returns_the_smoothed_people(gpu_caffe, synth152, kind, stages):
    net = _net(kind, gpu_caffe, synth152[0])
    kw = dict(scale=1.0, **CHAIN)
    kw.update(stages)
    net.forward_images(FRAMES[0], 1.0, want=(), pose=False)
    want = net.assemble_people(**kw)[0]
    _check_entry(gpu_caffe, want, lambda t: net.track_people(t, **kw)[0])


@pytest.mark.parametrize("stages", STAGES, ids=STAGE_IDS)
@pytest.mark.parametrize("mirrored", [False, True], ids=["plain", "mirrored"])
def test_group_track_people_returns_the_smoothed_people(gpu_caffe, synth152, mirrored, stages):
    from pose import MIRROR_MPII14
    from pose.estimate_pose import _scale_group

    net = _net("f32", gpu_caffe, synth152[0])
    scales = [1.0, 0.7] * (2 if mirrored else 1)
    flags = [0, 0, 1, 1] if mirrored else None
    grp = _scale_group(net, len(scales))
    kw = dict(CHAIN)
    kw.update(stages)
    if mirrored:
        kw.update(mirror=flags, image_width=IMG.shape[1], joint_mirror=MIRROR_MPII14)
    grp.forward_images(FRAMES[0], scales, want=(), pose=False, mirror=flags)
    want = grp.assemble_people(scales, 0, **kw)[0]
    _check_entry(gpu_caffe, want, lambda t: grp.track_people(t, scales, 0, **kw)[0])


@pytest.mark.parametrize("stages", STAGES, ids=STAGE_IDS)
def test_track_frames_async_returns_the_smoothed_people(gpu_caffe, synth152, stages):
    net = _net("f32", gpu_caffe, synth152[0])
    kw = dict(CHAIN)
    kw.update(stages)
    net.forward_images(FRAMES[0], 1.0, want=(), pose=False)
    want = net.assemble_people(scale=1.0, **kw)[0]
    _check_entry(gpu_caffe, want, lambda t: net.track_frames_async(FRAMES[0], t, 1.0, **kw).result()[0])


@pytest.mark.parametrize("stages", STAGES, ids=STAGE_IDS)
def test_video_pipeline_passes_the_smoothed_people_through(gpu_caffe, synth152, stages):
    """VideoPipeline(depth=2, batch=2) over four frames of one sequence: the people are those of a second, identically seeded tracker fed
    assemble_people's people frame by frame, bit for bit, the first frame's planted joint bridged; the ids are those of a tracker without
    smoothing, whose pipeline returns assemble_people's people."""
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    kw = dict(CHAIN)
    kw.update(stages)
    want = []
    for i in (0, 2):
        net.forward_images(np.stack(FRAMES[i:i + 2]), 1.0, want=(), pose=False)
        want += net.assemble_people(scale=1.0, **kw)
    first = want[0]["people"]
    on, q, j = _seeded(gpu_caffe, first, SKW)
    by_hand, _, _ = _seeded(gpu_caffe, first, SKW)
    off, _, _ = _seeded(gpu_caffe, first, None)
    runs = {}
    for name, tracker in (("on", on), ("off", off)):
        pipe = VideoPipeline(net, tracker, depth=2, batch=2, stats=(EDGES, MEAN, STD), choose_streams=False, **dict(AKW, **stages))
        for k, f in enumerate(FRAMES):
            pipe.submit(f, tag=k)
        runs[name] = pipe.drain()
        assert pipe.calls == 2 and [t for t, _, _ in runs[name]] == [0, 1, 2, 3]
    differs = 0
    for k, w in enumerate(want):
        m = len(w["people"])
        ids, _, smooth, src = by_hand.update([w["people"]], return_smooth=True)
        assert np.array_equal(runs["on"][k][1], smooth[0, :m]) and np.array_equal(runs["on"][k][2], ids[0, :m])
        assert np.array_equal(runs["off"][k][1], w["people"]) and np.array_equal(runs["off"][k][2], runs["on"][k][2])
        differs += int((smooth[0, :m] != w["people"]).any())
        if k == 0:
            assert src[0, q, j] == 2 and runs["on"][0][1][q, j, 2] == 0.5 and w["people"][q, j, 2] == 0.0
    assert differs >= 1 and sum(len(w["people"]) for w in want) > 0
    a, b = on.smooth_state(), by_hand.smooth_state()
    assert all(np.array_equal(a[k], b[k]) for k in a)

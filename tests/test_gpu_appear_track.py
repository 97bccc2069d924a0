"""GPU: the tracker's appearance steps (dc_tracker_update_appearance) against their restatement in tests/appear_ref.py, EXACTLY: ids, place,
reid, the tracks' models and the gallery after every frame — the steps are integer, so there is no tolerance.  `dist` is bit for bit what
a plain tracker gives on the same frames, and with smoothing on so are the smoothed poses.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; the rule is this project's own.

Scenes use dyadic coordinates, and `_arrays` asserts in the restatement that every pose distance is at least 1e-9 away from max_dist, so
that no pose decision hangs on a rounding; the appearance decisions need no margin."""
import functools

import numpy as np
import pytest

import appear_ref as AR
import assign_ref as AS
import track_ref as TR

pytestmark = pytest.mark.gpu

J = 3
TRACK = dict(max_misses=2, min_common=1, max_dist=0.5, min_size=16.0, motion=0)
PRM = TR.params(J, **TRACK)
AP = AR.appearance_params(min_pixels=10, alpha256=64, reid_max=3000, max_age=12, min_hits=2)
SMOOTH = dict(min_cutoff=0.125, beta=2.0, d_cutoff=0.0625, max_hold=2)
AWAY = TRACK["max_misses"] + 3


def _pose(x, y):
    return np.array([[x, y, 0.9], [x + 8.0, y, 0.9], [x + 4.0, y + 16.0, 0.9]])


def _colour(bin_, n=200):
    h = np.zeros((3, 16), np.int32)
    h[:, bin_ % 16], h[:, (bin_ + 1) % 16] = n - n // 4, n // 4
    return h


def _arrays(frames, T, P, ap=AP, assign="greedy", with_desc=True):
    """frames: per frame a list of (x, y, colour bin[, pixels]) -> people [F, P, J, 3], n [F], desc [F, P, 3, 16] and what the restatement
    gives per frame: (ids, place, reid, the appearance state, the tracks' ids).  Asserts the distance margin."""
    F = len(frames)
    ppl, n, desc = np.zeros((F, P, J, 3)), np.zeros(F, np.int32), np.zeros((F, P, 3, 16), np.int32)
    slot, app, want = TR.Slot(T, J), AR.Appearance(T), []
    for f, people in enumerate(frames):
        n[f] = len(people)
        for k, person in enumerate(people):
            ppl[f, k], desc[f, k] = _pose(person[0], person[1]), _colour(*person[2:])
        ids, place, reid, D = AR.update(slot, app, ppl[f], int(n[f]), P, PRM, ap, desc[f] if with_desc else None,
                                        AS.associate if assign == "optimal" else TR.associate)
        finite = D[np.isfinite(D)]
        assert finite.size == 0 or np.abs(finite - PRM["max_dist"]).min() >= 1e-9, "a pose distance within 1e-9 of max_dist"
        want.append((ids, place, reid, AR.appearance_state(slot, app), TR.state(slot)[0]))
    return ppl, n, desc, want


def _tracker(caffe, T, assign="greedy", smooth=None, appearance=AP, slots=1):
    return caffe.Tracker(n_joints=J, slots=slots, max_tracks=T, assign=assign, smooth=smooth, appearance=appearance, **TRACK)


def _same_state(got, want, where):
    for k, w in zip(("track_model", "track_valid", "gallery_ids", "gallery_age", "gallery_model"), want):
        assert np.array_equal(got[k], w), (where, k, np.argwhere(got[k] != w)[:4].tolist())


def _drive(caffe, frames, T, P, assign="greedy", smooth=None, ap=AP):
    """The device, frame by frame, against the restatement and against a plain tracker -> the restatement's results."""
    ppl, n, desc, want = _arrays(frames, T, P, ap, assign)
    t, plain = _tracker(caffe, T, assign, smooth, ap), _tracker(caffe, T, assign, smooth, None)
    for f in range(len(frames)):
        out = t.update(ppl[f][None], n_people=n[f:f + 1], desc=desc[f][None], return_dist=True, return_reid=True, return_smooth=smooth is not None)
        ref = plain.update(ppl[f][None], n_people=n[f:f + 1], return_dist=True, return_smooth=smooth is not None)
        ids, place, reid, state, track_ids = want[f]
        assert np.array_equal(out[0][0], ids), (f, out[0][0], ids)
        assert np.array_equal(out[1][0], place) and np.array_equal(out[1], ref[1]), (f, out[1][0], place)
        assert np.array_equal(out[-1][0], reid), (f, out[-1][0], reid)
        assert out[2].tobytes() == ref[2].tobytes(), (f, "dist")
        if smooth is not None:
            assert out[3].tobytes() == ref[3].tobytes() and np.array_equal(out[4], ref[4]), (f, "step 8")
        _same_state(t.appearance_state(0), state, f)
        assert np.array_equal(t.state(0)["ids"], track_ids), f
    return want


# ---- the scripted sequences at T = P = 4 ----------------------------------------------------------------------------------------------
def test_a_person_who_comes_back_elsewhere_takes_the_old_id(gpu_caffe):
    frames = [[(10.0, 10.0, 2), (100.0, 10.0, 9)]] * 3 + [[(100.0, 10.0, 9)]] * AWAY + [[(100.0, 10.0, 9), (60.0, 90.0, 2)]] * 2
    want = _drive(gpu_caffe, frames, 4, 4)
    assert want[3 + AWAY][0][:2].tolist() == [1, 0] and want[3 + AWAY][2][:2].tolist() == [0, 1]
    assert (want[-1][3][2] == -1).all()  # the gallery is empty again


def test_another_colour_does_not_take_the_id_and_an_old_entry_is_gone(gpu_caffe):
    want = _drive(gpu_caffe, [[(10.0, 10.0, 2)]] * 3 + [[]] * AWAY + [[(60.0, 90.0, 11)]], 4, 4)
    assert want[-1][0][0] == 1 and want[-1][2][0] == 0 and sorted(want[-1][3][2].tolist())[-1] == 0  # id 0 still waits
    for extra, last in ((AP["max_age"] - 1, (0, 1)), (AP["max_age"], (1, 0))):
        want = _drive(gpu_caffe, [[(10.0, 10.0, 2)]] * 3 + [[]] * (TRACK["max_misses"] + 1 + extra) + [[(60.0, 90.0, 2)]], 4, 4)
        assert (int(want[-1][0][0]), int(want[-1][2][0])) == last, extra
    # fewer hits than min_hits; fewer pixels than min_pixels
    assert _drive(gpu_caffe, [[(10.0, 10.0, 2)]] + [[]] * AWAY + [[(60.0, 90.0, 2)]], 4, 4)[-1][0][0] == 1
    assert _drive(gpu_caffe, [[(10.0, 10.0, 2, 9)]] * 3 + [[]] * AWAY + [[(60.0, 90.0, 2, 9)]], 4, 4)[-1][0][0] == 1


def test_two_returning_people_and_one_entry_the_closer_colour_wins_and_no_place_free(gpu_caffe):
    """Two people return at once with colours near one entry: the pair with the smaller A takes it (7' 's order), the other gets a new
    id; a fifth person finds no free place and stays untracked (id -1) with or without a descriptor."""
    frames = [[(10.0, 10.0, 4, 200)]] * 3 + [[]] * AWAY + [[(200.0, 90.0, 4, 161), (60.0, 90.0, 4, 200), (300.0, 10.0, 9), (400.0, 10.0, 12),
                                                            (500.0, 10.0, 4)]]
    want = _drive(gpu_caffe, frames, 4, 5)
    ids, reid = want[-1][0].tolist(), want[-1][2].tolist()
    assert ids[4] == -1 and reid == [0, 1, 0, 0, 0] and ids[:4] == [1, 0, 2, 3]  # A = 18 for 161 pixels, 0 for 200


# ---- the gallery overflows ------------------------------------------------------------------------------------------------------------
def test_seventy_tracks_freed_in_one_update_overflow_the_gallery(gpu_caffe):
    T = P = 128
    ap = dict(AP, min_hits=1)

    def crowd(first, count):
        return [(64.0 * (k % 16), 64.0 * (k // 16), k % 16, 100 + k) for k in range(first, first + count)]

    frames = [crowd(0, 30)] + [[]] * (TRACK["max_misses"] + 1) + [crowd(30, 70)] + [[]] * (TRACK["max_misses"] + 1)
    ppl, n, desc, _ = _arrays(frames, T, P, ap)
    # the second crowd in two bins five apart, half the pixels each: at least 3072 away from every `_colour`, beyond reid_max
    at = TRACK["max_misses"] + 2
    for k in range(70):
        desc[at, k] = 0
        desc[at, k][:, (30 + k) % 16], desc[at, k][:, (30 + k + 5) % 16] = 50, 50
    slot, app, t = TR.Slot(T, J), AR.Appearance(T), _tracker(gpu_caffe, T, appearance=ap)
    for f in range(len(frames)):
        ids, place, reid, _D = AR.update(slot, app, ppl[f], int(n[f]), P, PRM, ap, desc[f])
        got = t.update(ppl[f][None], n_people=n[f:f + 1], desc=desc[f][None], return_reid=True)
        assert np.array_equal(got[0][0], ids) and np.array_equal(got[1][0], place) and np.array_equal(got[2][0], reid) and not reid.any(), f
        _same_state(t.appearance_state(0), AR.appearance_state(slot, app), f)
    gi = t.appearance_state(0)["gallery_ids"].tolist()
    # 70 freed at once into 34 free entries; the other 36 replace the oldest: entries 0 .. 29 in turn, then — every age is 0 — entry 0 again
    assert gi[30:] == list(range(30, 64)) and gi[1:30] == list(range(65, 94)) and gi[0] == 99


# ---- every combination of matching rule and smoothing ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _walk(seed=7, frames=26, people=6):
    """Six people of six colours on a dyadic grid, each walking a few sixteenths per frame and away for stretches longer than
    max_misses; when they come back they stand somewhere else."""
    rs = np.random.RandomState(seed)
    home = [(96.0 * k, 32.0 * (k % 2)) for k in range(people)]
    gone_from = [int(rs.randint(3, 10)) for _ in range(people)]
    gone_for = [int(rs.randint(AWAY, AWAY + 5)) for _ in range(people)]
    out = []
    for f in range(frames):
        here = []
        for k in range(people):
            if gone_from[k] <= f < gone_from[k] + gone_for[k]:
                continue
            back = f >= gone_from[k] + gone_for[k]
            x, y = home[k][0] + (640.0 if back else 0.0) + 0.0625 * f * (k + 1), home[k][1] + (200.0 if back else 0.0) + 0.125 * f
            here.append((x, y, 2 * k + 1, 150 + 10 * k + (f % 3)))
        order = rs.permutation(len(here))
        out.append(tuple(here[i] for i in order))
    return tuple(out)


@pytest.mark.parametrize("smooth", [None, SMOOTH], ids=["raw", "smoothed"])
@pytest.mark.parametrize("assign", ["greedy", "optimal"])
def test_every_matching_rule_and_smoothing_with_appearance_on(gpu_caffe, assign, smooth):
    want = _drive(gpu_caffe, [list(f) for f in _walk()], 8, 8, assign, smooth)
    assert sum(int(w[2].sum()) for w in want) >= 4  # people came back and took their ids
    assert max(int(w[0].max()) for w in want) == 5  # ... so six ids served the whole walk


# ---- several images of one slot in one call; the older entries ------------------------------------------------------------------------
def test_six_images_of_one_slot_in_one_call_equal_six_calls(gpu_caffe):
    frames = [list(f) for f in _walk()][6:24]
    ppl, n, desc, want = _arrays(frames, 8, 8)
    one, many = _tracker(gpu_caffe, 8, slots=2), _tracker(gpu_caffe, 8, slots=2)
    for f0 in range(0, len(frames), 6):
        got = many.update(ppl[f0:f0 + 6], n_people=n[f0:f0 + 6], desc=desc[f0:f0 + 6], slot_of=[1] * 6, return_dist=True, return_reid=True)
        for k in range(6):
            ref = one.update(ppl[f0 + k][None], n_people=n[f0 + k:f0 + k + 1], desc=desc[f0 + k][None], slot_of=[1], return_dist=True, return_reid=True)
            for a, b in zip(got, ref):
                assert a[k].tobytes() == b[0].tobytes(), (f0, k)
            assert np.array_equal(ref[0][0], want[f0 + k][0]) and np.array_equal(ref[3][0], want[f0 + k][2])
        _same_state(many.appearance_state(1), want[f0 + 5][3], f0)
        _same_state(one.appearance_state(1), want[f0 + 5][3], f0)
    assert (many.appearance_state(0)["gallery_ids"] == -1).all() and (many.state(0)["ids"] == -1).all()  # the other slot is untouched


def test_without_descriptors_the_ids_are_the_plain_trackers_and_the_lifecycle(gpu_caffe):
    frames = [list(f) for f in _walk()]
    ppl, n, desc, blind = _arrays(frames, 8, 8, with_desc=False)
    t, plain = _tracker(gpu_caffe, 8), _tracker(gpu_caffe, 8, appearance=None)
    for f in range(len(frames)):
        got, ref = t.update(ppl[f][None], n_people=n[f:f + 1], return_dist=True), plain.update(ppl[f][None], n_people=n[f:f + 1], return_dist=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, ref)), f
        assert np.array_equal(got[0][0], blind[f][0]) and not blind[f][2].any()
        _same_state(t.appearance_state(0), blind[f][3], f)  # nobody has a valid model, so nothing enters the gallery
    assert not t.appearance_state(0)["track_valid"].any() and (t.appearance_state(0)["gallery_ids"] == -1).all()
    # desc=None through the appearance entry is the same thing
    t2 = _tracker(gpu_caffe, 8)
    for f in range(8):
        got = t2.update(ppl[f][None], n_people=n[f:f + 1], return_reid=True)
        assert np.array_equal(got[0][0], blind[f][0]) and not got[2].any()
    # lifecycle: a parameter change while on keeps models and gallery; reset clears them; off -> on starts empty
    t3 = _tracker(gpu_caffe, 8)
    ppl, n, desc, want = _arrays(frames, 8, 8)
    upto = next(f for f in range(len(frames)) if (want[f][3][2] >= 0).any() and want[f][3][1].any())
    for f in range(upto + 1):
        t3.update(ppl[f][None], n_people=n[f:f + 1], desc=desc[f][None])
    _same_state(t3.appearance_state(0), want[upto][3], "before the change")
    t3.appearance = dict(AP, reid_max=2999)
    _same_state(t3.appearance_state(0), want[upto][3], "after a parameter change")
    t3.appearance = None
    t3.appearance = AP
    st = t3.appearance_state(0)
    assert not st["track_valid"].any() and (st["gallery_ids"] == -1).all() and (t3.state(0)["ids"] >= 0).any()  # the tracks stay
    t3.update(ppl[upto + 1][None], n_people=n[upto + 1:upto + 2], desc=desc[upto + 1][None])
    assert t3.appearance_state(0)["track_valid"].any()
    t3.reset()
    st = t3.appearance_state(0)
    assert not st["track_valid"].any() and (st["gallery_ids"] == -1).all() and (t3.state(0)["ids"] == -1).all()


# ---- pose.track_people(appearance=) ---------------------------------------------------------------------------------------------------
from test_gpu_track import AKW, EDGES, FRAMES, MEAN, STD, TKW, _net, cost_model_tiles  # noqa: E402,F401  (the fixture: cost-model tiles)


@pytest.mark.parametrize("smooth", [None, True], ids=["raw", "smoothed"])
def test_pose_track_people_with_appearance_is_the_four_calls_by_hand(gpu_caffe, synth152, smooth):
    """Per frame: the forward, `assemble_people`, `describe_people` on the frame, `Tracker.update(people, desc=...)`; with smoothing on the
    smoothed poses are yielded.  The tracker of the caller gets its `appearance` from the dict's tracker keys."""
    from pose import TORSO_MPII14, track_people

    net = _net("f32", gpu_caffe, synth152[0])
    frames, stats = FRAMES + FRAMES[:1], (EDGES, MEAN, STD)
    tracker = gpu_caffe.Tracker(n_joints=14, smooth=smooth, **TKW)
    got = list(track_people(frames, None, None, stats, tracker=tracker, net=net, appearance=dict(scale=0.1, min_pixels=1, min_hits=1), **AKW))
    assert tracker.appearance == dict({k: gpu_caffe.APPEARANCE_DEFAULTS[k] for k in ("alpha256", "reid_max", "max_age")}, min_pixels=1, min_hits=1)
    by_hand = gpu_caffe.Tracker(n_joints=14, smooth=smooth, appearance=dict(min_pixels=1, min_hits=1), **TKW)
    assert len(got) == len(frames) and sum(len(p) for p, _ in got) > 0
    for frame, (people, ids) in zip(frames, got):
        net.forward_images(frame, 1.0, want=(), pose=False)
        raw = net.assemble_people(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **AKW)[0]["people"]
        m = len(raw)
        assert len(people) == m and ids.shape == (m,) and ids.dtype == np.int64
        if m == 0:  # the tracker is still updated: its tracks miss
            by_hand.update(np.zeros((1, 1, 14, 3)), n_people=[0], desc=np.zeros((1, 1, 3, 16), np.int32))
            continue
        desc = gpu_caffe.describe_people(frame, raw, edges=TORSO_MPII14, scale=0.1)
        out = by_hand.update(raw[None], desc=desc[None], return_smooth=smooth is not None)
        assert np.array_equal(ids, out[0][0]) and np.array_equal(people, out[2][0] if smooth else raw)

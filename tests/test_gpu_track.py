"""-m gpu: the tracker (dc_tracker_update and the chained dc_net_track_people / dc_group_track_people, csrc/track.hip) against the
float64 restatement of the rule in tests/track_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker, so there is no reference output to hold the
kernel to.  The rule is this project's own (include/deepcut_hip.h, dc_tracker_update); what is proven here is that the device computes
what the restatement computes: the distances to 1e-9 * max(1, |D|) — the bound the pair costs are held to —, and everything decided from
them (ids, places, the slots' state) bit for bit when the restated steps 4-7 run on the device's own distances."""
import numpy as np
import pytest

import people_ref as R
import track_ref as TR

pytestmark = pytest.mark.gpu

J = 14


def _random_people(rs, n, lo=0.0, hi=500.0, p_missing=0.25):
    """n people of J joints around random centres: x, y, score; a missing joint is (0, 0, 0)."""
    out = np.zeros((n, J, 3), np.float64)
    for q in range(n):
        c = rs.uniform(lo + 60, hi - 60, 2)
        out[q, :, :2] = c + rs.uniform(-50, 50, (J, 2))
        out[q, :, 2] = rs.uniform(0.1, 1.0, J)
        out[q, rs.rand(J) < p_missing] = 0.0
    return out


def _jitter(rs, people, sd, p_flip=0.1):
    """The same people a frame later: every held joint moved by N(0, sd), a few joints appearing / vanishing."""
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


def _same_state(tracker, slots):
    for b, slot in enumerate(slots):
        st = tracker.state(b)
        ids, misses, hits, poses = TR.state(slot)
        assert np.array_equal(st["ids"], ids) and np.array_equal(st["misses"], misses) and np.array_equal(st["hits"], hits), b
        assert np.array_equal(st["poses"], poses), b


def _step_on_device_dist(tracker, slots, prm, frames, P):
    """One update of every slot on the device; the restated steps 4-7 then run on the DEVICE's own distances and must decide the same.
    -> (ids, place, dist) of the device."""
    ppl, n = _pack(frames, P)
    ids, place, dist = tracker.update(ppl, n, return_dist=True)
    for b, slot in enumerate(slots):
        rid, rplace = TR.associate(slot, dist[b], ppl[b], int(n[b]), P, prm)
        assert np.array_equal(ids[b], rid) and np.array_equal(place[b], rplace), b
    _same_state(tracker, slots)
    return ids, place, dist


@pytest.mark.parametrize("motion", [0, 1])
def test_distances_match_the_restatement(gpu_caffe, motion):
    """S = 3, T = 20, P = 24 (T * P = 480 > 256: every strided loop of the kernel takes a second trip), random poses with missing
    joints, a random sigma; after two warm-up updates, so that velocities and misses are not trivial."""
    S, T, P = 3, 20, 24
    rs = np.random.RandomState(11 + motion)
    sigma = rs.uniform(0.5, 2.0, J)
    kw = dict(max_misses=3, min_common=3, max_dist=0.02, min_size=20.0, motion=motion)
    tracker = gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, sigma=sigma, **kw)
    prm = TR.params(J, sigma, **kw)
    slots = [TR.Slot(T, J) for _ in range(S)]
    world = [_random_people(rs, n) for n in (15, 24, 10)]  # slot 1: more people than places
    _step_on_device_dist(tracker, slots, prm, world, P)
    for step in range(2):
        frames = []
        for b in range(S):
            world[b] = _jitter(rs, world[b], 4.0)
            keep = rs.permutation(len(world[b]))[: len(world[b]) - 2 * (step == 0)]  # warm-up 1 hides two people: their tracks miss
            frames.append(world[b][keep])
        if step == 0:
            _step_on_device_dist(tracker, slots, prm, frames, P)
    ppl, n = _pack(frames, P)
    want = [TR.distances(slots[b], ppl[b], int(n[b]), P, prm) for b in range(S)]
    assert any(s.misses[i] > 0 for s in slots for i in range(T) if s.live[i]) and any(np.abs(s.vel).max() > 0 for s in slots)
    _, _, got = tracker.update(ppl, n, return_dist=True)
    assert got.shape == (S, T, P)
    worst, finite = 0.0, 0
    for b in range(S):
        assert not np.isnan(got[b]).any() and not np.isneginf(got[b]).any()
        assert np.array_equal(np.isposinf(got[b]), np.isposinf(want[b]))
        fin = np.isfinite(want[b])
        finite += int(fin.sum())
        worst = max(worst, float((np.abs(got[b][fin] - want[b][fin]) / np.maximum(1.0, np.abs(want[b][fin]))).max()))
    print("track distances, motion %d: %d finite of %d, max |device - restatement| / max(1, |D|) = %.3e" % (motion, finite, S * T * P, worst))
    assert finite > 300 and finite < S * T * P
    assert worst <= 1e-9


def _random_sequence(tracker, seed, S, T, P, prm, updates=12):
    rs = np.random.RandomState(seed)
    slots = [TR.Slot(T, J) for _ in range(S)]
    world = [_random_people(rs, 6), _random_people(rs, 9)]
    log = []
    for u in range(updates):
        frames = []
        for b in range(S):
            w = _jitter(rs, world[b], 3.0)
            w = w[rs.rand(len(w)) > 0.12]  # people vanish for good ...
            if rs.rand() < 0.6 and len(w) < P:  # ... and appear
                w = np.concatenate([w, _random_people(rs, 1 + int(rs.rand() < 0.3 and len(w) + 1 < P))])
            world[b] = w
            hidden = rs.rand(len(w)) < 0.15  # and some are missed for a frame
            frames.append(w[~hidden][rs.permutation(int((~hidden).sum()))])  # in any order
        ids, place, dist = _step_on_device_dist(tracker, slots, prm, frames, P)
        st = [tracker.state(b) for b in range(S)]
        log.append((ids, place, dist, st))
    return log, slots


def test_matching_bit_for_bit_on_a_random_sequence(gpu_caffe):
    """12 updates of S = 2 with jitter, people appearing, vanishing, hidden for a frame and reordered: at every update ids, place and the
    state equal the restated steps 4-7 run on the device's own distances; the sequence a second time on a fresh tracker gives the same."""
    S, T, P = 2, 10, 12
    kw = dict(max_misses=2, min_common=3, max_dist=0.03, min_size=20.0, motion=1)
    prm = TR.params(J, None, **kw)
    runs = []
    for _ in range(2):
        tracker = gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, **kw)
        runs.append(_random_sequence(tracker, 5, S, T, P, prm))
    (a, slots), (b, _) = runs
    for (ia, pa, da, sa), (ib, pb, db, sb) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(pa, pb) and np.array_equal(da, db)
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(sa, sb) for k in x)
    # the sequence did what it is there for: births after the first frame, deaths, matches over several frames
    assert slots[0].next_id > 6 and slots[1].next_id > 9 and any(not all(s.live) and s.next_id > T for s in slots)
    assert any((ids >= 0).sum() > 0 for ids, _, _, _ in a[1:]) and max(int(h["hits"].max()) for _, _, _, st in a for h in st) >= 4


# ---- planted walkers ------------------------------------------------------------------------------------------------------------
SKELETON = np.array([(-20, 40), (-20, 20), (-20, 0), (20, 0), (20, 20), (20, 40), (-30, -10), (-30, -30), (-20, -40), (20, -40), (30, -30),
                     (30, -10), (0, -45), (0, -60)], np.float64)  # integer offsets: extent 60 x 100 pixels, s = 100


def _walker(cx, cy):
    p = np.zeros((J, 3), np.float64)
    p[:, 0], p[:, 1], p[:, 2] = SKELETON[:, 0] + cx, SKELETON[:, 1] + cy, 0.75
    return p


def _walk(gap, frames, hide=None):
    """Three walkers on integer-pixel paths: A walks right and B left at 6 pixels a frame, `gap` pixels apart in y, crossing in the
    middle of the sequence; C stands still, far away.  hide = (walker, first, count): that walker is not seen for `count` frames.
    -> per frame: (the people, in an order that changes from frame to frame; which walker each of them is)."""
    out = []
    for f in range(frames):
        who = [0, 1, 2]
        pos = {0: (200 + 6 * f, 300), 1: (200 + 6 * (frames - 1) - 6 * f, 300 + gap), 2: (900, 700)}
        if hide is not None and hide[1] <= f < hide[1] + hide[2]:
            who.remove(hide[0])
        who = who[f % len(who):] + who[: f % len(who)]
        out.append((np.stack([_walker(*pos[w]) for w in who]), who))
    return out


PLANT = dict(max_misses=3, min_common=3, max_dist=0.05, min_size=20.0)


def _run_planted(gpu_caffe, motion, gap, hide, frames=17):
    seq = _walk(gap, frames, hide)
    prm = TR.params(J, None, motion=motion, **PLANT)
    # the restatement alone, before the device is consulted
    slot, gaps, ref = TR.Slot(8, J), {}, []
    for people, who in seq:
        ids, place, _ = TR.update(slot, people, len(people), 4, prm, gaps)
        ref.append((ids, place, who))
    print("planted walkers, motion %d, gap %d, hide %r: gap between a chosen match and the best one it rules out >= %.6g, gap to max_dist "
          ">= %.6g" % (motion, gap, hide, gaps["choice"], gaps["max_dist"]))
    assert gaps["choice"] >= 1e-6 and gaps["max_dist"] >= 1e-6
    # then the device
    tracker = gpu_caffe.Tracker(n_joints=J, slots=1, max_tracks=8, motion=motion, **PLANT)
    for (people, who), (ids, place, _) in zip(seq, ref):
        ppl, n = _pack([people], 4)
        got_ids, got_place = tracker.update(ppl, n)
        assert np.array_equal(got_ids[0], ids) and np.array_equal(got_place[0], place)
    _same_state(tracker, [slot])
    by_walker = {}
    for ids, _, who in ref:
        for q, w in enumerate(who):
            by_walker.setdefault(w, []).append(int(ids[q]))
    return by_walker


@pytest.mark.parametrize("motion,gap", [(1, 8), (0, 24)], ids=["motion1_narrow_crossing", "motion0_wide_crossing"])
def test_planted_walkers_keep_their_ids(gpu_caffe, motion, gap):
    """Two walkers cross, a third stands still: the restatement alone gives every walker one id throughout, with every greedy choice at
    least 1e-6 from the best match it rules out and every distance at least 1e-6 from max_dist — so a 1e-9 difference in a distance
    cannot flip a choice —, and then the device agrees at every frame.  Motion 1 predicts the walkers' constant velocity exactly, so the
    crossing may be 8 pixels narrow; motion 0 compares with the last pose, and its variant crosses 24 pixels apart."""
    by_walker = _run_planted(gpu_caffe, motion, gap, None)
    assert all(len(set(v)) == 1 and v[0] >= 0 for v in by_walker.values()) and len({v[0] for v in by_walker.values()}) == 3


@pytest.mark.parametrize("motion", [0, 1])
def test_hidden_walker_returns(gpu_caffe, motion):
    """Hidden for max_misses updates, the standing walker returns with its id; hidden for max_misses + 1 it returns with a new one, and
    the old id never reappears."""
    gap = 8 if motion else 24
    back = _run_planted(gpu_caffe, motion, gap, (2, 5, PLANT["max_misses"]))
    assert len(set(back[2])) == 1 and all(len(set(v)) == 1 for v in back.values())
    gone = _run_planted(gpu_caffe, motion, gap, (2, 5, PLANT["max_misses"] + 1))
    old, new = gone[2][0], gone[2][-1]
    assert gone[2] == [old] * 5 + [new] * (len(gone[2]) - 5) and new == 3 and old not in gone[0] + gone[1]
    assert len(set(gone[0])) == 1 and len(set(gone[1])) == 1


# ---- ties -------------------------------------------------------------------------------------------------------------------------
def _square(x, y):
    """4 joints on a 4-pixel square: s = max(min_size = 4, 4) = 4, every coordinate a small integer, so every distance is exact"""
    return np.array([(x, y, 0.5), (x + 4, y, 0.5), (x, y + 4, 0.5), (x + 4, y + 4, 0.5)], np.float64)


@pytest.mark.parametrize("motion", [0, 1])
def test_ties_go_to_the_lower_place_then_the_lower_person(gpu_caffe, motion):
    kw = dict(max_misses=5, min_common=1, max_dist=1.0, min_size=4.0, motion=motion)
    prm = TR.params(4, None, **kw)

    def run(first, second):
        tracker = gpu_caffe.Tracker(n_joints=4, slots=1, max_tracks=4, **kw)
        slot = TR.Slot(4, 4)
        for people in (first, second):
            ppl = np.stack(people)[None]
            ids, place, dist = tracker.update(ppl, return_dist=True)
            rid, rplace, rdist = TR.update(slot, ppl[0], len(people), len(people), prm)
            assert np.array_equal(dist[0], rdist)  # exact: small integers and powers of two
            assert np.array_equal(ids[0], rid) and np.array_equal(place[0], rplace)
        return ids[0], place[0], dist[0], tracker.state(0)

    # two people equidistant from one track: the lower q wins, whichever side it is on
    for a, b in ((10, 6), (6, 10)):
        ids, place, dist, st = run([_square(8, 8)], [_square(a, 8), _square(b, 8)])
        assert dist[0, 0] == dist[0, 1] == 0.25
        assert list(ids) == [0, 1] and list(place) == [0, 1]
    # two tracks equidistant from one person, at D == max_dist exactly: the lower place wins, the other track misses
    ids, place, dist, st = run([_square(8, 8), _square(16, 8)], [_square(12, 8)])
    assert dist[0, 0] == dist[1, 0] == 1.0
    assert list(ids) == [0] and list(place) == [0] and list(st["misses"][:2]) == [0, 1] and list(st["hits"][:2]) == [2, 1]
    # all four distances equal: (place 0, person 0) first, then (1, 1)
    ids, place, dist, st = run([_square(8, 8), _square(16, 8)], [_square(12, 8), _square(12, 8)])
    assert (dist[:2, :2] == 1.0).all() and list(ids) == [0, 1] and list(place) == [0, 1]


# ---- capacity ---------------------------------------------------------------------------------------------------------------------
def test_capacity_reuse_empty_frames_and_reset(gpu_caffe):
    kw = dict(max_misses=0, min_common=1, max_dist=1.0, min_size=4.0, motion=1)
    prm = TR.params(4, None, **kw)
    tracker = gpu_caffe.Tracker(n_joints=4, slots=2, max_tracks=2, **kw)
    slots = [TR.Slot(2, 4), TR.Slot(2, 4)]
    a, b, c, d = _square(8, 8), _square(108, 8), _square(208, 8), _square(308, 8)
    # T = 2 with three people: the third gets -1; slot 1 alike
    ids, place, _ = _step_on_device_dist(tracker, slots, prm, [np.stack([a, b, c]), np.stack([a, b, c])], 3)
    assert ids.tolist() == [[0, 1, -1], [0, 1, -1]] and place.tolist() == [[0, 1, -1], [0, 1, -1]]
    # b's track dies (max_misses = 0) and its place is reused in the same update, with a fresh id; the untracked c was never given one
    ids, place, _ = _step_on_device_dist(tracker, slots, prm, [np.stack([d, a]), np.stack([a, b])], 3)
    assert ids[0].tolist() == [2, 0, -1] and place[0].tolist() == [1, 0, -1] and ids[1].tolist() == [0, 1, -1]
    # n = 0: every track misses (and, max_misses being 0, dies)
    ids, place, _ = _step_on_device_dist(tracker, slots, prm, [np.zeros((0, 4, 3)), np.stack([a, b])], 3)
    assert (ids[0] == -1).all() and (tracker.state(0)["ids"] == -1).all() and tracker.state(1)["ids"].tolist() == [0, 1]
    # reset(1) leaves slot 0 alone (its next id is 3) and restarts slot 1 at 0
    tracker.reset(1)
    slots[1].reset()
    _same_state(tracker, slots)
    ids, place, _ = _step_on_device_dist(tracker, slots, prm, [np.stack([a]), np.stack([b])], 3)
    assert ids[0].tolist() == [3, -1, -1] and ids[1].tolist() == [0, -1, -1]
    tracker.reset()
    assert all((tracker.state(s)["ids"] == -1).all() and not tracker.state(s)["poses"].any() for s in (0, 1))


def test_full_size_update_equals_the_restatement(gpu_caffe):
    """T = P = n = 256 once: 256 people of 3 joints on a 100-pixel grid, forty of them in pairs 10 pixels apart, born in one update and
    matched, jittered and reordered, in the next — in which one person of ten of the pairs has gone far away: the track it leaves behind
    has its nearest person taken by the neighbour's track (its row minimum is re-derived, and nothing is left), and the person, every
    place being taken, gets -1."""
    T = P = 256
    kw = dict(max_misses=1, min_common=2, max_dist=0.5, min_size=20.0, motion=1)
    prm = TR.params(3, None, **kw)
    rs = np.random.RandomState(3)
    centres = np.array([(100.0 * (k % 16) + 50, 100.0 * (k // 16) + 50) for k in range(256)])
    for k in range(0, 40, 2):
        centres[k + 1] = centres[k] + (10, 0)
    tri = np.array([(0, 0), (20, 0), (0, 20)], np.float64)
    first = np.zeros((256, 3, 3))
    first[:, :, :2], first[:, :, 2] = centres[:, None, :] + tri, 0.5
    perm = rs.permutation(256)
    second = first.copy()
    second[:, :, :2] += rs.uniform(-3, 3, (256, 3, 2))
    moved = np.arange(1, 20, 2)
    second[moved, :, :2] += 5000.0
    second = second[perm]
    tracker = gpu_caffe.Tracker(n_joints=3, slots=1, max_tracks=T, **kw)
    slot = TR.Slot(T, 3)
    ids, _, _ = _step_on_device_dist(tracker, [slot], prm, [first], P)
    assert ids[0].tolist() == list(range(256))
    want = TR.distances(slot, second, 256, P, prm)
    ids, place, dist = _step_on_device_dist(tracker, [slot], prm, [second], P)
    assert np.isfinite(want).all() and np.array_equal(np.isposinf(dist[0]), np.isposinf(want))
    assert (np.abs(dist[0] - want) / np.maximum(1.0, np.abs(want))).max() <= 1e-9
    assert ((want <= 0.5).sum(1) >= 2).sum() >= 20  # tracks with more than one person in reach
    assert ids[0].tolist() == [-1 if k in moved else int(k) for k in perm]
    assert tracker.state()["misses"][moved].tolist() == [1] * 10


# ---- chains -----------------------------------------------------------------------------------------------------------------------
H, W = 200, 264
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))
EDGES = R.all_pairs_edges()
AKW = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(3)]
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


def _net(kind, caffe, path):
    from deepcut_tools import deepercut_prototxt

    if kind not in _nets:
        kw = {"f32": dict(), "f16": dict(dtype="f16"), "sparse": dict(want=["loc_pred", "prob"], sparse_pairwise=True)}[kind]
        _nets[kind] = caffe.Net(deepercut_prototxt(152, H, W), path, caffe.TEST, from_text=True, **kw)
    return _nets[kind]


def _check_chain(caffe, forward, track, assemble):
    """Three forwards: the chained entry returns what the assembly entry returns on the same forward, and its ids are those of a second
    tracker fed the returned people through Tracker.update."""
    chained, by_hand = caffe.Tracker(n_joints=J, **TKW), caffe.Tracker(n_joints=J, **TKW)
    seen, total = set(), 0
    for k, frame in enumerate(FRAMES):
        forward(frame)
        got = track(chained)
        want = assemble()
        assert len(got) == len(want) == 1
        g, w = got[0], want[0]
        assert len(g["people"]) == len(w["people"]) and np.array_equal(g["people"], w["people"]) and np.array_equal(g["cand"], w["cand"])
        m = len(g["people"])
        assert g["ids"].shape == (m,) and g["place"].shape == (m,) and g["ids"].dtype == np.int64
        ids, place = by_hand.update([g["people"]])
        assert np.array_equal(ids[0, :m], g["ids"]) and np.array_equal(place[0, :m], g["place"])
        assert (g["ids"] >= 0).all() and len(set(g["ids"].tolist())) == m
        seen |= set(g["ids"].tolist())
        total += m
        a, b = chained.state(), by_hand.state()
        assert all(np.array_equal(a[key], b[key]) for key in a)
    print("chain: %d people over %d frames, %d distinct ids" % (total, len(FRAMES), len(seen)))
    assert total > 0


@pytest.mark.parametrize("kind", ["f32", "f16", "sparse"])
def test_net_track_people_is_assemble_people_plus_ids(gpu_caffe, synth152, kind):
    net = _net(kind, gpu_caffe, synth152[0])
    assert net.dtype == ("f16" if kind == "f16" else "f32")
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **AKW)
    _check_chain(gpu_caffe, lambda f: net.forward_images(f, 1.0, want=(), pose=False), lambda t: net.track_people(t, **kw),
                 lambda: net.assemble_people(**kw))


@pytest.mark.parametrize("mirrored", [False, True], ids=["plain", "mirrored"])
def test_group_track_people_is_assemble_people_plus_ids(gpu_caffe, synth152, mirrored):
    from pose import MIRROR_MPII14
    from pose.estimate_pose import _scale_group

    net = _net("f32", gpu_caffe, synth152[0])
    scales = [1.0, 0.7] * (2 if mirrored else 1)
    flags = [0, 0, 1, 1] if mirrored else None
    grp = _scale_group(net, len(scales))
    kw = dict(edges=EDGES, mean=MEAN, std=STD, **AKW)
    if mirrored:
        kw.update(mirror=flags, image_width=IMG.shape[1], joint_mirror=MIRROR_MPII14)
    _check_chain(gpu_caffe, lambda f: grp.forward_images(f, scales, want=(), pose=False, mirror=flags), lambda t: grp.track_people(t, scales, 0, **kw),
                 lambda: grp.assemble_people(scales, 0, **kw))


def test_pose_track_people_over_frames(gpu_caffe, synth152):
    """pose.track_people over three frames, the second a caffe.Frame.nv12: per frame what forward_images + Net.track_people give by hand,
    and the people are estimate_people's."""
    from pose import estimate_people, track_people

    net = _net("f32", gpu_caffe, synth152[0])
    rs = np.random.RandomState(9)
    h, w = IMG.shape[:2]
    y, uv = rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, ((h + 1) // 2, (w + 1) // 2, 2)).astype(np.uint8)
    frames = [FRAMES[0], gpu_caffe.Frame.nv12(y, uv), FRAMES[1]]
    stats = (EDGES, MEAN, STD)
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    got = list(track_people(frames, None, None, stats, tracker=tracker, net=net, **AKW))
    assert len(got) == 3
    by_hand = gpu_caffe.Tracker(n_joints=J, **TKW)
    for frame, (people, ids) in zip(frames, got):
        net.forward_images(frame, 1.0, want=(), pose=False)
        want = net.track_people(by_hand, scale=1.0, edges=EDGES, mean=MEAN, std=STD, **AKW)[0]
        assert np.array_equal(people, want["people"]) and np.array_equal(ids, want["ids"]) and ids.dtype == np.int64
        assert np.array_equal(people, estimate_people(frame, None, None, stats, net=net, **AKW))
    assert sum(len(p) for p, _ in got) > 0
    # the default tracker is made on the first frame; a pyramid goes through the group's entry
    one = list(track_people(frames[:1], None, None, stats, net=net, scales=[1.0, 0.7], **AKW))
    assert len(one) == 1 and np.array_equal(one[0][0], estimate_people(frames[0], None, None, stats, net=net, scales=[1.0, 0.7], **AKW))
    assert one[0][1].shape == (len(one[0][0]),)

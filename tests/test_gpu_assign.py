"""-m gpu: step 4' of the tracking rule — the optimal assignment of a frame's people to a slot's live tracks (match_optimal in
csrc/track.hip, chosen by DC_TRACK_OPT_ASSIGN / `caffe.Tracker(assign="optimal")`) — against its float64 restatement in
tests/assign_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker.  The rule is this project's own
(include/deepcut_hip.h, dc_tracker_update) and it is a procedure, scan order included; what is proven here is that the device decides
what the restated procedure decides, bit for bit (ids, places, the slots' state), when the restatement runs on the device's own
distances — whose agreement with the restated steps 1-3 is tests/test_gpu_track.py's business, and step 4' does not touch them."""
import copy

import numpy as np
import pytest

import assign_ref as AR
import people_ref as R
import track_ref as TR

pytestmark = pytest.mark.gpu

J = 14
RULES = {"greedy": TR.associate, "optimal": AR.associate}


def _random_people(rs, n, lo=0.0, hi=500.0, p_missing=0.25, joints=J):
    """n people around random centres: x, y, score; a missing joint is (0, 0, 0)."""
    out = np.zeros((n, joints, 3), np.float64)
    for q in range(n):
        c = rs.uniform(lo + 60, hi - 60, 2)
        out[q, :, :2] = c + rs.uniform(-50, 50, (joints, 2))
        out[q, :, 2] = rs.uniform(0.1, 1.0, joints)
        out[q, rs.rand(joints) < p_missing] = 0.0
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


def _step(tracker, slots, prm, frames, P, rule="optimal", count=None):
    """One update of every slot on the device; the restated matching of `rule` and steps 5-7 then run on the DEVICE's own distances and
    must decide the same.  -> (ids, place, dist) of the device."""
    assert tracker.assign == rule
    ppl, n = _pack(frames, P)
    ids, place, dist = tracker.update(ppl, n, return_dist=True)
    for b, slot in enumerate(slots):
        kw = {"count": count} if rule == "optimal" and count is not None else {}
        rid, rplace = RULES[rule](slot, dist[b], ppl[b], int(n[b]), P, prm, **kw)
        assert np.array_equal(ids[b], rid) and np.array_equal(place[b], rplace), (b, ids[b], rid)
    _same_state(tracker, slots)
    return ids, place, dist


def _square(x, y):
    """4 joints on a 4-pixel square: s = max(min_size = 4, 4) = 4, every coordinate a small integer, so every distance is exact"""
    return np.array([(x, y, 0.5), (x + 4, y, 0.5), (x, y + 4, 0.5), (x + 4, y + 4, 0.5)], np.float64)


# ---- 1. what the option is for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", [0, 1])
def test_two_people_passing_keep_their_ids(gpu_caffe, motion):
    """Tracks born at x = 8 and x = 16, then people at x = 2 and x = 10: D = [[2.25, 0.25], [12.25, 2.25]] exactly.  Greedy takes 0.25
    first and has to accept 12.25 — both identities swap, total 12.5; the assignment that keeps both costs 4.5."""
    kw = dict(max_misses=5, min_common=1, max_dist=16.0, min_size=4.0, motion=motion)
    prm = TR.params(4, None, **kw)
    got = {}
    for rule in ("greedy", "optimal"):
        tracker = gpu_caffe.Tracker(n_joints=4, slots=1, max_tracks=4, assign=rule, **kw)
        slot = TR.Slot(4, 4)
        ids, _, _ = _step(tracker, [slot], prm, [np.stack([_square(8, 8), _square(16, 8)])], 2, rule)
        assert ids[0].tolist() == [0, 1]
        ids, place, dist = _step(tracker, [slot], prm, [np.stack([_square(2, 8), _square(10, 8)])], 2, rule)
        assert np.array_equal(dist[0, :2], np.array([[2.25, 0.25], [12.25, 2.25]])) and np.isposinf(dist[0, 2:]).all()
        got[rule] = ids[0].tolist()
        assert place[0].tolist() == got[rule]  # the places are the ids here
    assert got == {"greedy": [1, 0], "optimal": [0, 1]}


# ---- 2. random sequences ------------------------------------------------------------------------------------------------------------
BODY = np.array([(-20, 40), (-20, 20), (-20, 0), (20, 0), (20, 20), (20, 40), (-30, -10), (-30, -30), (-20, -40), (20, -40), (30, -30),
                 (30, -10), (0, -45), (0, -60)], np.float64)  # integer offsets: extent 60 x 100 pixels, s = 100


def _grid_people(rs, n):
    """n rigid bodies with every joint held, centres on an 8-pixel grid inside 96 x 96 pixels: D = |centre - centre|^2 / 100^2 for every
    pair, a sum of 14 equal terms whatever the pair — equal offsets give bit-equal distances"""
    out = np.zeros((n, J, 3), np.float64)
    out[:, :, :2] = BODY + 8.0 * rs.randint(0, 13, (n, 1, 2)) + 200.0
    out[:, :, 2] = 0.5
    return out


def _random_sequence(tracker, seed, S, T, P, prm, grid, updates=12):
    rs = np.random.RandomState(seed)
    slots = [TR.Slot(T, J) for _ in range(S)]
    make = _grid_people if grid else _random_people
    world = [make(rs, 6), make(rs, 9)]
    log, count, ties = [], {}, 0
    for u in range(updates):
        frames = []
        for b in range(S):
            if grid:
                w = world[b].copy()
                w[:, :, :2] += 8.0 * rs.randint(-1, 2, (len(w), 1, 2))
            else:
                w = _jitter(rs, world[b], 3.0)
            w = w[rs.rand(len(w)) > 0.12]  # people vanish for good ...
            if rs.rand() < 0.6 and len(w) < P:  # ... and appear
                w = np.concatenate([w, make(rs, 1 + int(rs.rand() < 0.3 and len(w) + 1 < P))])
            world[b] = w
            hidden = rs.rand(len(w)) < 0.15  # and some are missed for a frame
            frames.append(w[~hidden][rs.permutation(int((~hidden).sum()))])  # in any order
        ids, place, dist = _step(tracker, slots, prm, frames, P, "optimal", count)
        allowed = dist[dist <= prm["max_dist"]]
        ties += allowed.size - np.unique(allowed).size
        log.append((ids, place, dist, [tracker.state(b) for b in range(S)]))
    return log, slots, count["trips"], ties


@pytest.mark.parametrize("grid", [False, True], ids=["jittered", "integer_grid_ties"])
def test_matching_bit_for_bit_on_a_random_sequence(gpu_caffe, grid):
    """12 updates of S = 2, T = 10, P = 12 with jitter, people appearing, vanishing, hidden for a frame and reordered: at every update
    ids, place and the state equal the restated steps 4', 5-7 run on the device's own distances; the sequence a second time on a fresh
    tracker gives the same.  The second variant puts rigid bodies on an 8-pixel grid in a small field, so that many allowed distances
    are bit-equal and the scan order of the procedure decides."""
    S, T, P = 2, 10, 12
    kw = dict(max_misses=2, min_common=3, max_dist=0.2 if grid else 0.03, min_size=20.0, motion=1)
    prm = TR.params(J, None, **kw)
    runs = []
    for _ in range(2):
        tracker = gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, assign="optimal", **kw)
        runs.append(_random_sequence(tracker, 5, S, T, P, prm, grid))
    (a, slots, trips, ties), (b, _, _, _) = runs
    for (ia, pa, da, sa), (ib, pb, db, sb) in zip(a, b):
        assert np.array_equal(ia, ib) and np.array_equal(pa, pb) and np.array_equal(da, db)
        assert all(np.array_equal(x[k], y[k]) for x, y in zip(sa, sb) for k in x)
    print("optimal assignment, random sequence (%s): %d inner trips over 24 matchings, %d allowed distances equal to another one"
          % ("grid" if grid else "jittered", trips, ties))
    # the sequence did what it is there for: births after the first frame, deaths, matches over several frames — and ties where asked for
    assert slots[0].next_id + slots[1].next_id > 6 + 9
    assert any((ids >= 0).sum() > 0 for ids, _, _, _ in a[1:]) and max(int(h["hits"].max()) for _, _, _, st in a for h in st) >= 3
    assert ties >= 20 or not grid


# ---- 3. the gate --------------------------------------------------------------------------------------------------------------------
def test_the_gate_and_the_capacity(gpu_caffe):
    """A pair at D == max_dist exactly ties with a dummy column and is matched (the real column comes first in the scan); the same pair
    is not matched by a tracker whose max_dist is the next double below; n = 0; more people than free places; every place free."""
    kw = dict(max_misses=5, min_common=1, max_dist=1.0, min_size=4.0, motion=0)
    for max_dist, matched in ((1.0, True), (float(np.nextafter(1.0, 0.0)), False)):
        k = dict(kw, max_dist=max_dist)
        prm = TR.params(4, None, **k)
        tracker = gpu_caffe.Tracker(n_joints=4, slots=1, max_tracks=3, assign="optimal", **k)
        slot = TR.Slot(3, 4)
        # every place free: R = 0, two births
        ids, place, dist = _step(tracker, [slot], prm, [np.stack([_square(8, 8), _square(108, 8)])], 4)
        assert ids[0].tolist() == [0, 1, -1, -1] and np.isposinf(dist).all()
        # D == 1.0 for (track 0, person 0); person 1 is nobody's
        ids, place, dist = _step(tracker, [slot], prm, [np.stack([_square(12, 8), _square(300, 8)])], 4)
        assert dist[0, 0, 0] == 1.0 and dist[0, 1, 0] == 576.0
        assert ids[0].tolist() == ([0, 2, -1, -1] if matched else [2, -1, -1, -1])  # unmatched: one free place, person 0 is born into it
        assert tracker.state()["misses"].tolist() == ([0, 1, 0] if matched else [1, 1, 0])
        # n = 0: every track misses
        ids, place, _ = _step(tracker, [slot], prm, [np.zeros((0, 4, 3))], 4)
        assert (ids == -1).all() and (place == -1).all() and min(tracker.state()["misses"].tolist()) == 1
        # four people, three live tracks and no free place: the matched keep their ids, the others get -1 and nothing is born
        where = tracker.state()["poses"][:, 0, 0]
        frame = np.stack([_square(where[2] + 1, 8), _square(500, 8), _square(where[0] - 1, 8), _square(700, 8)])
        next_id = slot.next_id
        ids, place, _ = _step(tracker, [slot], prm, [frame], 4)
        assert ids[0].tolist() == [slot.id[2], -1, slot.id[0], -1] and place[0].tolist() == [2, -1, 0, -1] and slot.next_id == next_id


# ---- 4. past the first trip of every loop -------------------------------------------------------------------------------------------
def _contended(gpu_caffe, T, P, first, second, seed, area, sd, max_dist):
    """`first` people are born, then `second` people arrive: the first ones moved by N(0, sd) a joint and reordered, the rest new.
    -> (ids of the second update, inner trips of its matching, the greedy total and the optimal total on the device's distances)"""
    kw = dict(max_misses=3, min_common=3, max_dist=max_dist, min_size=20.0, motion=1)
    prm = TR.params(J, None, **kw)
    rs = np.random.RandomState(seed)
    tracker = gpu_caffe.Tracker(n_joints=J, slots=1, max_tracks=T, assign="optimal", **kw)
    slot = TR.Slot(T, J)
    world = _random_people(rs, first, 0.0, area)
    ids, _, _ = _step(tracker, [slot], prm, [world], P)
    assert ids[0, :first].tolist() == list(range(first))
    moved = _jitter(rs, world, sd)
    if second > first:
        moved = np.concatenate([moved, _random_people(rs, second - first, 0.0, area)])
    moved = moved[rs.permutation(second)]
    before, count = copy.deepcopy(slot), {}
    ids, place, dist = _step(tracker, [slot], prm, [moved], P, count=count)
    opt = AR.assign(dist[0], before.live, second, kw["max_dist"])
    greedy = copy.deepcopy(before)
    gid, gplace = TR.associate(greedy, dist[0], moved, second, P, prm)
    gpairs = {int(gplace[q]): q for q in range(second) if gid[q] >= 0 and gid[q] < first}
    totals = AR.total(dist[0], before.live, gpairs, kw["max_dist"]), AR.total(dist[0], before.live, opt, kw["max_dist"])
    return ids[0], count["trips"], totals, gpairs != opt


def test_forty_tracks_against_forty_eight_people(gpu_caffe):
    """m = 88: more than one wave of columns, real and dummy columns in the same wave, eight births behind the matching."""
    ids, trips, (greedy, optimal), differs = _contended(gpu_caffe, 48, 48, 40, 48, 21, 200.0, 40.0, 1.5)
    print("40 x 48: %d inner trips; total greedy %.6f optimal %.6f; the matchings differ: %s" % (trips, greedy, optimal, differs))
    assert trips > 40 and optimal < greedy and differs and sorted(ids.tolist()) == list(range(48))


def test_a_second_column_per_thread(gpu_caffe):
    """150 live tracks against 150 people: m = 300, threads 0..43 own a second (dummy) column."""
    ids, trips, (greedy, optimal), differs = _contended(gpu_caffe, 150, 150, 150, 150, 22, 400.0, 30.0, 1.0)
    print("150 x 150: %d inner trips; total greedy %.6f optimal %.6f; the matchings differ: %s" % (trips, greedy, optimal, differs))
    assert trips > 150 and optimal < greedy and differs


def test_full_size_near(gpu_caffe):
    """T = P = n = 256, m = 512, in the near arrangement of test_gpu_track.py's full-size test: 256 people of 3 joints on a 100-pixel
    grid, forty of them in pairs 10 pixels apart, jittered and reordered in the second update, in which one person of ten of the pairs
    has gone far away.  The track it leaves behind could take the neighbour's person for 0.25 and leave the neighbour's track unmatched
    for 0.5; keeping the neighbour and paying 0.5 for itself costs less, so it misses, and the person, every place taken, gets -1."""
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
    tracker = gpu_caffe.Tracker(n_joints=3, slots=1, max_tracks=T, assign="optimal", **kw)
    slot = TR.Slot(T, 3)
    ids, _, _ = _step(tracker, [slot], prm, [first], P)
    assert ids[0].tolist() == list(range(256))
    count = {}
    ids, place, dist = _step(tracker, [slot], prm, [second], P, count=count)
    print("T = P = n = 256, near: %d inner trips" % count["trips"])
    assert ((dist[0] <= 0.5).sum(1) >= 2).sum() >= 20  # tracks with more than one person in reach
    assert ids[0].tolist() == [-1 if k in moved else int(k) for k in perm]
    assert tracker.state()["misses"][moved].tolist() == [1] * 10


def test_full_size_random(gpu_caffe):
    """T = P = n = 256 once on 256 uniformly random poses against 256 others, every pair allowed: thousands of inner trips, long
    augmenting paths, every thread's two columns in use."""
    T = P = 256
    kw = dict(max_misses=1, min_common=2, max_dist=1e9, min_size=20.0, motion=0)
    prm = TR.params(3, None, **kw)
    rs = np.random.RandomState(8)
    tracker = gpu_caffe.Tracker(n_joints=3, slots=1, max_tracks=T, assign="optimal", **kw)
    slot = TR.Slot(T, 3)
    frames = [_random_people(rs, 256, 0.0, 3000.0, 0.0, 3) for _ in range(2)]
    _step(tracker, [slot], prm, frames[:1], P)
    count = {}
    ids, _, dist = _step(tracker, [slot], prm, frames[1:], P, count=count)
    print("T = P = n = 256, random: %d inner trips" % count["trips"])
    assert sorted(ids[0].tolist()) == list(range(256)) and ids[0].tolist() != list(range(256)) and count["trips"] > 1000


# ---- 5. slot map, 6. switching ------------------------------------------------------------------------------------------------------
def test_three_frames_in_one_call_equal_three_calls(gpu_caffe):
    S, T, P = 2, 10, 12
    kw = dict(max_misses=2, min_common=3, max_dist=0.2, min_size=20.0, motion=1)
    prm = TR.params(J, None, **kw)
    rs = np.random.RandomState(31)
    world = _grid_people(rs, 8)
    frames = []
    for _ in range(3):
        world = world.copy()
        world[:, :, :2] += 8.0 * rs.randint(-1, 2, (len(world), 1, 2))
        frames.append(world[rs.permutation(8)[:7]])
    one, three = [gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, assign="optimal", **kw) for _ in range(2)]
    ppl, n = _pack(frames, P)
    ids, place, dist = one.update(ppl, n, return_dist=True, slot_of=[1, 1, 1])
    slots = [TR.Slot(T, J), TR.Slot(T, J)]
    for b in range(3):
        i3, p3, d3 = three.update(ppl[b:b + 1], n[b:b + 1], return_dist=True, slot_of=[1])
        assert np.array_equal(i3[0], ids[b]) and np.array_equal(p3[0], place[b]) and np.array_equal(d3[0], dist[b])
        rid, rplace = AR.associate(slots[1], dist[b], ppl[b], int(n[b]), P, prm)
        assert np.array_equal(ids[b], rid) and np.array_equal(place[b], rplace)
    _same_state(one, slots)
    _same_state(three, slots)
    assert slots[0].next_id == 0 and int(one.state(1)["hits"].max()) == 3


def test_switching_the_rule_between_updates(gpu_caffe):
    """Greedy for two updates, optimal for the next, greedy again, on people who keep moving left by 6 pixels with their neighbour 8
    pixels away (motion 0): every update equals the restatement of the rule in force on the state the one before left — the greedy
    updates swap the two ids, the optimal one does not."""
    kw = dict(max_misses=5, min_common=1, max_dist=16.0, min_size=4.0, motion=0)
    prm = TR.params(4, None, **kw)
    tracker = gpu_caffe.Tracker(n_joints=4, slots=1, max_tracks=4, **kw)
    slot = TR.Slot(4, 4)
    seen = []
    for x, rule in ((14, "greedy"), (8, "greedy"), (2, "optimal"), (-4, "greedy")):
        if tracker.assign != rule:
            tracker.assign = rule
        ids, _, _ = _step(tracker, [slot], prm, [np.stack([_square(x, 8), _square(x + 8, 8)])], 2, rule)
        seen.append(ids[0].tolist())
    assert seen == [[0, 1], [1, 0], [1, 0], [0, 1]]


# ---- 7. chains ----------------------------------------------------------------------------------------------------------------------
H, W = 200, 264
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))
EDGES = R.all_pairs_edges()
AKW = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1, assign="optimal")
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(3)]


@pytest.fixture(scope="module")
def net(gpu_caffe, synth152):
    """The small synthetic ResNet-152 in float32, tiles from the cost model (DC_AUTOTUNE=0: nothing is timed)."""
    import os

    from deepcut_tools import deepercut_prototxt

    old = os.environ.get("DC_AUTOTUNE")
    os.environ["DC_AUTOTUNE"] = "0"
    yield gpu_caffe.Net(deepercut_prototxt(152, H, W), synth152[0], gpu_caffe.TEST, from_text=True)
    if old is None:
        del os.environ["DC_AUTOTUNE"]
    else:
        os.environ["DC_AUTOTUNE"] = old


def _check_chain(caffe, forward, track, assemble):
    """Three forwards: the chained entry returns what the assembly entry returns on the same forward, and its ids are those of a second
    optimal tracker fed the returned people through Tracker.update.  -> the chained results"""
    chained, by_hand = caffe.Tracker(n_joints=J, **TKW), caffe.Tracker(n_joints=J, **TKW)
    out = []
    for frame in FRAMES:
        forward(frame)
        got = track(chained)
        want = assemble()
        assert len(got) == len(want) == 1
        g, w = got[0], want[0]
        assert np.array_equal(g["people"], w["people"]) and np.array_equal(g["cand"], w["cand"])
        m = len(g["people"])
        ids, place = by_hand.update([g["people"]])
        assert np.array_equal(ids[0, :m], g["ids"]) and np.array_equal(place[0, :m], g["place"])
        assert (g["ids"] >= 0).all() and len(set(g["ids"].tolist())) == m
        a, b = chained.state(), by_hand.state()
        assert all(np.array_equal(a[key], b[key]) for key in a)
        out.append(g)
    assert sum(len(g["people"]) for g in out) > 0 and int(chained.state()["hits"].max()) >= 2
    return out


def test_net_chain_and_async_entry_with_an_optimal_tracker(gpu_caffe, net):
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **AKW)
    sync = _check_chain(gpu_caffe, lambda f: net.forward_images(f, 1.0, want=(), pose=False), lambda t: net.track_people(t, **kw),
                        lambda: net.assemble_people(**kw))
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    for frame, want in zip(FRAMES, sync):
        got = net.track_frames_async(frame, tracker, 1.0, edges=EDGES, mean=MEAN, std=STD, **AKW).result()[0]
        assert all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in ("people", "cand", "ids", "place"))
    assert tracker.assign == "optimal"


def test_group_chain_with_an_optimal_tracker(gpu_caffe, net):
    from pose.estimate_pose import _scale_group

    scales = [1.0, 0.7]
    grp = _scale_group(net, len(scales))
    kw = dict(edges=EDGES, mean=MEAN, std=STD, **AKW)
    _check_chain(gpu_caffe, lambda f: grp.forward_images(f, scales, want=(), pose=False), lambda t: grp.track_people(t, scales, 0, **kw),
                 lambda: grp.assemble_people(scales, 0, **kw))

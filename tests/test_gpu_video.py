"""-m gpu: several images per tracker slot in one launch (the slot map of dc_tracker_update_slots, dc_net_track_people_slots,
csrc/track.hip) against the same images applied one per call, and against the float64 restatement of the rule in tests/track_ref.py.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps and has no tracker, so there is no reference output to hold the
kernel to.  The rule is this project's own (include/deepcut_hip.h, dc_tracker_update).  The slot map is DEFINED as applying the images of
a slot one at a time in ascending order, so every comparison here is bit for bit (np.array_equal): there is no tolerance to choose."""
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


# ---- the slot map on host poses -----------------------------------------------------------------------------------------------------
S, T, P = 4, 20, 24  # T * P = 480 > 256: every strided loop of the kernel takes a second trip
SLOT_OF = [2, 0, 2, 1, 0, 2, 2]
MAP_KW = dict(max_misses=1, min_common=3, max_dist=0.02, min_size=20.0, motion=1)
MAP_SEED = 2


def _map_calls(seed=MAP_SEED):
    """Two calls of nb = 7 images with SLOT_OF: every slot has a world of people that move from image to image, are hidden for an image,
    leave for good and arrive.  -> (sigma, [frames of call 0, frames of call 1])"""
    rs = np.random.RandomState(seed)
    sigma = rs.uniform(0.5, 2.0, J)
    world = {0: _random_people(rs, 9), 1: _random_people(rs, 5), 2: _random_people(rs, 12)}
    calls = []
    for _ in range(2):
        frames = []
        for s in SLOT_OF:
            w = _jitter(rs, world[s], 4.0)
            w = w[rs.rand(len(w)) > 0.1]
            if rs.rand() < 0.7:
                w = np.concatenate([w, _random_people(rs, 1)])
            world[s] = w
            hidden = rs.rand(len(w)) < 0.2
            frames.append(w[~hidden][rs.permutation(int((~hidden).sum()))])
        calls.append(frames)
    return sigma, calls


def _slot2_did_its_job(sigma, calls):
    """The restatement alone over slot 2's images: between its images WITHIN one call there is a match of a track with non-zero velocity,
    a live track that misses and a birth."""
    prm = TR.params(J, sigma, **MAP_KW)
    slot = TR.Slot(T, J)
    seen = dict(moving_match=0, miss=0, birth=0)
    for frames in calls:
        first = True
        for b, s in enumerate(SLOT_OF):
            if s != 2:
                continue
            live, vel, misses, next_id = np.array(slot.live).copy(), np.array(slot.vel).copy(), np.array(slot.misses).copy(), slot.next_id
            ids, place, _ = TR.update(slot, _pack([frames[b]], P)[0][0], len(frames[b]), P, prm)
            if not first:  # the state this image saw was written by an image of the same call
                for q in range(len(frames[b])):
                    if place[q] >= 0 and ids[q] < next_id and live[place[q]] and np.abs(vel[place[q]]).max() > 0:
                        seen["moving_match"] += 1
                    if ids[q] >= next_id:
                        seen["birth"] += 1
                seen["miss"] += int(sum(1 for i in range(T) if live[i] and i not in set(place[: len(frames[b])].tolist()) and
                                        (not slot.live[i] or slot.misses[i] > misses[i])))
            first = False
    return seen


@pytest.fixture(scope="module")
def map_run(gpu_caffe):
    """The two calls on a tracker of S slots with the slot map, and the same images one per call on three trackers of one slot.
    -> dict: per call (ppl, n, ids, place, dist) of the mapped tracker, the yardstick's per image, the states."""
    sigma, calls = _map_calls()
    mapped = gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, sigma=sigma, **MAP_KW)
    single = {s: gpu_caffe.Tracker(n_joints=J, slots=1, max_tracks=T, sigma=sigma, **MAP_KW) for s in (0, 1, 2)}
    out = dict(sigma=sigma, calls=calls, got=[], want=[])
    for frames in calls:
        ppl, n = _pack(frames, P)
        ids, place, dist = mapped.update(ppl, n, return_dist=True, slot_of=SLOT_OF)
        out["got"].append((ppl, n, ids, place, dist))
        per_image = []
        for b, s in enumerate(SLOT_OF):
            i1, p1, d1 = single[s].update(ppl[b:b + 1], n[b:b + 1], return_dist=True)
            per_image.append((i1[0], p1[0], d1[0]))
        out["want"].append(per_image)
    out["state"] = [mapped.state(s) for s in range(S)]
    out["single_state"] = {s: single[s].state(0) for s in single}
    return out


def test_slot_map_equals_one_image_per_call(map_run):
    """nb = 7 images over slots [2, 0, 2, 1, 0, 2, 2] of a tracker of S = 4, two calls in a row: ids, place and dist of every image and
    the state of slots 0, 1, 2 equal those of three one-slot trackers fed the same images one per call; slot 3 is not touched."""
    seen = _slot2_did_its_job(map_run["sigma"], map_run["calls"])
    print("slot map, slot 2 between its images within a call: %r" % (seen,))
    assert seen["moving_match"] >= 1 and seen["miss"] >= 1 and seen["birth"] >= 1
    for (ppl, n, ids, place, dist), per_image in zip(map_run["got"], map_run["want"]):
        assert ids.shape == (7, P) and place.shape == (7, P) and dist.shape == (7, T, P)
        for b, (i1, p1, d1) in enumerate(per_image):
            assert np.array_equal(ids[b], i1) and np.array_equal(place[b], p1), b
            assert np.array_equal(dist[b], d1), b
    for s in (0, 1, 2):
        a, b = map_run["state"][s], map_run["single_state"][s]
        assert all(np.array_equal(a[k], b[k]) for k in a), s
        assert (a["ids"] >= 0).any()
    free = map_run["state"][3]
    assert (free["ids"] == -1).all() and not free["hits"].any() and not free["misses"].any() and not free["poses"].any()


def test_slot_map_next_id_of_an_unnamed_slot_stays_zero(gpu_caffe, map_run):
    """Slot 3 was named by no image of the two calls: the first person it ever sees gets id 0."""
    sigma, calls = map_run["sigma"], map_run["calls"]
    tracker = gpu_caffe.Tracker(n_joints=J, slots=S, max_tracks=T, sigma=sigma, **MAP_KW)
    for frames in calls:
        ppl, n = _pack(frames, P)
        tracker.update(ppl, n, slot_of=SLOT_OF)
    ids, _ = tracker.update(calls[0][0][None, :1], slot_of=[3])
    assert ids.tolist() == [[0]]


def test_slot_map_equals_the_restatement(map_run):
    """The same sequence through track_ref per slot in image order: steps 4-7 of the restatement, run on the device's own distances,
    decide the ids and places the device decided, and leave the state the device left."""
    prm = TR.params(J, map_run["sigma"], **MAP_KW)
    slots = [TR.Slot(T, J) for _ in range(S)]
    for ppl, n, ids, place, dist in map_run["got"]:
        for b, s in enumerate(SLOT_OF):
            rid, rplace = TR.associate(slots[s], dist[b], ppl[b], int(n[b]), P, prm)
            assert np.array_equal(ids[b], rid) and np.array_equal(place[b], rplace), b
    for s in range(S):
        st = map_run["state"][s]
        ids, misses, hits, poses = TR.state(slots[s])
        assert np.array_equal(st["ids"], ids) and np.array_equal(st["misses"], misses) and np.array_equal(st["hits"], hits), s
        assert np.array_equal(st["poses"], poses), s


def test_identity_map_is_update(gpu_caffe):
    """slot_of=None and slot_of=arange(nb) both give what Tracker.update gives on a second tracker, over three updates."""
    kw = dict(max_misses=2, min_common=3, max_dist=0.03, min_size=20.0, motion=1)
    rs = np.random.RandomState(21)
    trackers = [gpu_caffe.Tracker(n_joints=J, slots=3, max_tracks=10, **kw) for _ in range(3)]
    world = [_random_people(rs, 6), _random_people(rs, 9), _random_people(rs, 3)]
    for _ in range(3):
        world = [_jitter(rs, w, 3.0) for w in world]
        ppl, n = _pack([w[rs.permutation(len(w))[: len(w) - 1]] for w in world], 12)
        want = trackers[0].update(ppl, n, return_dist=True)
        none = trackers[1].update(ppl, n, return_dist=True, slot_of=None)
        ident = trackers[2].update(ppl, n, return_dist=True, slot_of=np.arange(3))
        for a, b, c in zip(want, none, ident):
            assert np.array_equal(a, b) and np.array_equal(a, c)
    for s in range(3):
        a, b, c = (t.state(s) for t in trackers)
        assert all(np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k]) for k in a)
    assert (trackers[0].state(1)["hits"] >= 3).any()


def test_full_size_two_images_in_one_slot(gpu_caffe):
    """T = P = n = 256, J = 3 once: the births of all 256 and a jittered, permuted second frame as two images of ONE call into one slot
    equal the two frames in two calls."""
    Tf = Pf = 256
    kw = dict(max_misses=1, min_common=2, max_dist=0.5, min_size=20.0, motion=1)
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
    one = gpu_caffe.Tracker(n_joints=3, slots=1, max_tracks=Tf, **kw)
    two = gpu_caffe.Tracker(n_joints=3, slots=1, max_tracks=Tf, **kw)
    ppl = np.stack([first, second])
    ids, place, dist = one.update(ppl, return_dist=True, slot_of=[0, 0])
    for b in range(2):
        i1, p1, d1 = two.update(ppl[b:b + 1], return_dist=True)
        assert np.array_equal(ids[b], i1[0]) and np.array_equal(place[b], p1[0]) and np.array_equal(dist[b], d1[0]), b
    assert ids[0].tolist() == list(range(256))
    assert ids[1].tolist() == [-1 if k in moved else int(k) for k in perm]
    a, b = one.state(), two.state()
    assert all(np.array_equal(a[k], b[k]) for k in a) and a["misses"][moved].tolist() == [1] * 10


# ---- chains -----------------------------------------------------------------------------------------------------------------------
H, W = 200, 264
STATS = np.random.RandomState(5)
MEAN, STD = STATS.randn(182, 2) * 15, STATS.uniform(4, 30, (182, 2))
EDGES = R.all_pairs_edges()
AKW = dict(threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2)
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)  # the rolled image of test_gpu_track.py: people persist
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(9)]
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


@pytest.mark.parametrize("kind", ["f32", "sparse"])
def test_chain_with_a_slot_map(gpu_caffe, synth152, kind):
    """A batch-3 forward of three frames of one video: Net.track_people(slot_of=[0, 0, 0]) returns assemble_people's people bit for bit,
    and its ids are those of a second tracker fed the returned people one frame at a time."""
    net = _net(kind, gpu_caffe, synth152[0])
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, **AKW)
    chained, by_hand = gpu_caffe.Tracker(n_joints=J, **TKW), gpu_caffe.Tracker(n_joints=J, **TKW)
    net.forward_images(np.stack(FRAMES[:3]), 1.0, want=(), pose=False)
    got = net.track_people(chained, slot_of=[0, 0, 0], **kw)
    want = net.assemble_people(**kw)
    assert len(got) == len(want) == 3
    total, persisted = 0, None
    for g, w in zip(got, want):
        assert np.array_equal(g["people"], w["people"]) and np.array_equal(g["cand"], w["cand"])
        m = len(g["people"])
        ids, place = by_hand.update([g["people"]])
        assert np.array_equal(ids[0, :m], g["ids"]) and np.array_equal(place[0, :m], g["place"])
        total += m
        persisted = set(g["ids"].tolist()) if persisted is None else persisted & set(g["ids"].tolist())
    a, b = chained.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    print("chain with a slot map (%s): %d people over 3 frames, %d ids in all three" % (kind, total, len(persisted)))
    assert total > 0 and int(a["hits"].max()) >= 2  # the second and third image saw the tracks the first one made


# ---- the asynchronous entry and frames in flight ------------------------------------------------------------------------------------
CHAIN = dict(edges=EDGES, mean=MEAN, std=STD, **AKW)


def _sync_path(caffe, net, frames, slots=None, n_slots=1):
    """The yardstick: forward_images + Net.track_people, one frame per call, on a fresh tracker -> (per-frame dicts, the tracker)."""
    tracker = caffe.Tracker(n_joints=J, slots=n_slots, **TKW)
    out = []
    for k, f in enumerate(frames):
        net.forward_images(f, 1.0, want=(), pose=False)
        out.append(net.track_people(tracker, scale=1.0, slot_of=None if slots is None else [slots[k]], **CHAIN)[0])
    return out, tracker


def _same(got, want, keys=("people", "cand", "ids", "place")):
    return all(np.array_equal(got[k], want[k]) and got[k].dtype == want[k].dtype for k in keys)


def _nv12_planes(k):
    rs = np.random.RandomState(30 + k)
    h, w = IMG.shape[:2]
    return rs.randint(0, 256, (h, w)).astype(np.uint8), rs.randint(0, 256, ((h + 1) // 2, (w + 1) // 2, 2)).astype(np.uint8)


@pytest.mark.parametrize("source", ["bgr", "nv12", "nv12_device"])
def test_async_entry_equals_the_synchronous_one(gpu_caffe, synth152, source):
    """Five frames through Net.track_frames_async, every result collected before the next submit, against forward_images +
    Net.track_people on a fresh tracker: people, cand, ids and place bit for bit.  How often the net was still busy right after the
    call returned is counted and printed, not asserted: the results are right whichever way that falls."""
    net = _net("f32", gpu_caffe, synth152[0])
    keep = []
    if source == "bgr":
        frames = FRAMES[:5]
    elif source == "nv12":
        y, uv = _nv12_planes(0)
        frames = [gpu_caffe.Frame.nv12(np.ascontiguousarray(np.roll(y, 8 * k, axis=1)), np.ascontiguousarray(np.roll(uv, 4 * k, axis=1)))
                  for k in range(5)]
    else:
        import torch

        y, uv = _nv12_planes(0)
        frames = []
        for k in range(5):
            ty = torch.from_numpy(np.ascontiguousarray(np.roll(y, 8 * k, axis=1))).cuda()
            tuv = torch.from_numpy(np.ascontiguousarray(np.roll(uv, 4 * k, axis=1))).cuda()
            keep.append((ty, tuv))
            frames.append(gpu_caffe.Frame.nv12_device(ty.data_ptr(), tuv.data_ptr(), y.shape[0], y.shape[1], y.shape[1], uv.shape[1] * 2))
        torch.cuda.synchronize()
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    got, busy = [], 0
    for f in frames:
        h = net.track_frames_async(f, tracker, 1.0, **CHAIN)
        busy += int(net.busy())
        got.append(h.result()[0])
        assert not net.busy() and h.done()
    want, by_hand = _sync_path(gpu_caffe, net, frames)
    print("async entry (%s): the net was busy right after %d of %d submits; %d people" % (source, busy, len(frames), sum(len(g["people"]) for g in got)))
    for g, w in zip(got, want):
        assert _same(g, w)
    a, b = tracker.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    assert sum(len(g["people"]) for g in got) > 0
    # without a tracker: assemble_people's people, no ids
    h = net.track_frames_async(frames[0], None, 1.0, **CHAIN)
    d = h.result()[0]
    assert set(d) == {"people", "cand"} and np.array_equal(d["people"], want[0]["people"]) and np.array_equal(d["cand"], want[0]["cand"])


def test_async_entry_on_the_sparse_pairwise_net(gpu_caffe, synth152):
    net = _net("sparse", gpu_caffe, synth152[0])
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    got = [net.track_frames_async(f, tracker, 1.0, **CHAIN).result()[0] for f in FRAMES[:3]]
    want, _ = _sync_path(gpu_caffe, net, FRAMES[:3])
    assert all(_same(g, w) for g, w in zip(got, want)) and sum(len(g["people"]) for g in got) > 0


def test_frames_in_flight_keep_their_order(gpu_caffe, synth152):
    """VideoPipeline(depth=3) over 9 frames of one sequence: every result is the synchronous path's, in submission order, ids persist,
    and a synchronous tracker.state() with requests in flight is the state after all submitted updates."""
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    want, by_hand = _sync_path(gpu_caffe, net, FRAMES)
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    pipe = VideoPipeline(net, tracker, depth=3, batch=1, stats=(EDGES, MEAN, STD), scale=1.0, **AKW)
    got = []
    for k, f in enumerate(FRAMES):
        pipe.submit(f, tag=k)
        while len(pipe._done):
            got.append(pipe.wait_one())
    in_flight = len(pipe._pending)
    a, b = tracker.state(), by_hand.state()  # requests are in flight: the state is the one after all of them
    assert in_flight >= 1 and all(np.array_equal(a[k], b[k]) for k in a)
    got += pipe.drain()
    assert [t for t, _, _ in got] == list(range(9))
    for (_, people, ids), w in zip(got, want):
        assert np.array_equal(people, w["people"]) and np.array_equal(ids, w["ids"]) and ids.dtype == np.int64
    runs = {}
    for _, _, ids in got:
        for i in ids.tolist():
            runs[i] = runs.get(i, 0) + 1
    print("frames in flight: %d people over 9 frames, %d ids, the longest-lived seen in %d frames; streams: %r" %
          (sum(len(p) for _, p, _ in got), len(runs), max(runs.values()), pipe.stream_choice))
    assert max(runs.values()) >= 3 and pipe.stream_choice is not None


def test_two_interleaved_sequences_in_flight(gpu_caffe, synth152):
    """Two sequences, frames alternating, on slots 0 and 1 of one tracker through VideoPipeline(depth=3)."""
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    other = [np.ascontiguousarray(np.roll(IMG[::-1], 8 * k, axis=1)) for k in range(4)]
    frames, slots = [], []
    for k in range(4):
        frames += [FRAMES[k], other[k]]
        slots += [0, 1]
    want, by_hand = _sync_path(gpu_caffe, net, frames, slots, n_slots=2)
    tracker = gpu_caffe.Tracker(n_joints=J, slots=2, **TKW)
    pipe = VideoPipeline(net, tracker, depth=3, stats=(EDGES, MEAN, STD), choose_streams=False, **AKW)
    for k, (f, s) in enumerate(zip(frames, slots)):
        pipe.submit(f, tag=k, slot=s)
    got = pipe.drain()
    assert [t for t, _, _ in got] == list(range(8))
    for (_, people, ids), w in zip(got, want):
        assert np.array_equal(people, w["people"]) and np.array_equal(ids, w["ids"])
    for s in (0, 1):
        a, b = tracker.state(s), by_hand.state(s)
        assert all(np.array_equal(a[k], b[k]) for k in a) and int(a["hits"].max()) >= 3


def test_batches_in_flight(gpu_caffe, synth152):
    """VideoPipeline(depth=2, batch=3) over 8 frames (the last batch is partial) against synchronous batch forwards + assemble_people,
    whose people go frame by frame to a second tracker."""
    from deepcut_tools import VideoPipeline

    net = _net("f32", gpu_caffe, synth152[0])
    frames = FRAMES[:8]
    by_hand = gpu_caffe.Tracker(n_joints=J, **TKW)
    want = []
    for i in range(0, 8, 3):
        net.forward_images(np.stack(frames[i:i + 3]), 1.0, want=(), pose=False)
        for d in net.assemble_people(scale=1.0, **CHAIN):
            ids, _ = by_hand.update([d["people"]])
            want.append((d["people"], ids[0, :len(d["people"])]))
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    pipe = VideoPipeline(net, tracker, depth=2, batch=3, stats=(EDGES, MEAN, STD), choose_streams=False, **AKW)
    for k, f in enumerate(frames):
        pipe.submit(f, tag=k)
    got = pipe.drain()
    assert pipe.calls == 3 and [t for t, _, _ in got] == list(range(8))
    for (_, people, ids), (wp, wi) in zip(got, want):
        assert np.array_equal(people, wp) and np.array_equal(ids, wi)
    a, b = tracker.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a) and sum(len(p) for _, p, _ in got) > 0


def test_pose_track_people_in_flight(gpu_caffe, synth152):
    """pose.track_people(depth=3) yields exactly what the default call yields; a pyramid with depth=3 is refused by name."""
    from pose import track_people

    net = _net("f32", gpu_caffe, synth152[0])
    stats = (EDGES, MEAN, STD)
    frames = FRAMES[:5]
    want = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=J, **TKW), net=net, **AKW))
    got = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=J, **TKW), net=net, depth=3, **AKW))
    both = list(track_people(frames, None, None, stats, tracker=gpu_caffe.Tracker(n_joints=J, **TKW), net=net, depth=2, batch=2, **AKW))
    assert len(got) == len(want) == 5 and sum(len(p) for p, _ in want) > 0
    for (p, i), (wp, wi) in zip(got, want):
        assert np.array_equal(p, wp) and np.array_equal(i, wi) and i.dtype == np.int64
    assert len(both) == 5 and all(len(p) == len(i) for p, i in both)
    for kw in (dict(scales=[1.0, 0.7]), dict(flip=True)):
        with pytest.raises(ValueError) as ei:
            list(track_people(frames[:1], None, None, stats, net=net, depth=3, **dict(AKW, **kw)))
        assert "depth" in str(ei.value) and "pyramid" in str(ei.value)


def test_pipelines_and_trackers_leave_no_device_memory_behind(gpu_caffe, synth152):
    """Create / submit / drain / destroy cycles of a pipeline with a tracker leave the free device memory where it was; and destroying a
    tracker whose last update was asynchronous waits for that update: its ids are in the host array when dc_tracker_destroy returns."""
    import gc

    import torch
    from deepcut_tools import VideoPipeline

    import caffe.pycaffe as pc

    net = _net("f32", gpu_caffe, synth152[0])
    dev = torch.device("cuda", 0)
    free = []
    for _ in range(4):  # the first cycle is the warm-up, three are measured
        tracker = gpu_caffe.Tracker(n_joints=J, slots=2, max_tracks=256, **TKW)
        pipe = VideoPipeline(net, tracker, depth=3, batch=2, stats=(EDGES, MEAN, STD), choose_streams=False, **AKW)
        for k, f in enumerate(FRAMES[:6]):
            pipe.submit(f, tag=k, slot=k % 2)
        assert len(pipe.drain()) == 6
        del pipe, tracker
        gc.collect()
        torch.cuda.synchronize(dev)
        free.append(torch.cuda.mem_get_info(dev)[0] / 2 ** 20)
    print("free device memory after each cycle, MiB: %r" % (free,))
    assert free[1] - free[-1] <= 2.0, free
    want, _ = _sync_path(gpu_caffe, net, FRAMES[:1])
    tracker = gpu_caffe.Tracker(n_joints=J, **TKW)
    h = net.track_frames_async(FRAMES[0], tracker, 1.0, **CHAIN)
    assert pc._lib.dc_tracker_destroy(tracker._h) == 0  # no wait of ours in between
    tracker._h = None
    m = len(want[0]["ids"])
    assert m > 0 and np.array_equal(h._ids[0, :m], want[0]["ids"]) and np.array_equal(h._place[0, :m], want[0]["place"])
    assert np.array_equal(h.result()[0]["people"], want[0]["people"])

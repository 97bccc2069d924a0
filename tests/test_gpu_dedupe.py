"""-m gpu: stage E of the people assembly, duplicate suppression (dedupe_kernel, csrc/people.hip; the rule: include/deepcut_hip.h,
dc_dedupe_params), against the float64 restatement in tests/dedupe_ref.py: alone through dc_dedupe_people on the crafted scenes of
tests/dedupe_scenes.py, and through every entry that assembles people.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps; like stages B to D and the tracker the rule is this project's
own, and what is proven here is that the device decides what the restatement decides.  Stage E copies values and computes only
decisions, so every comparison is for exact equality — of the bytes, for the poses, since some scenes carry NaNs.  What makes that
fair is a condition on the inputs (tests/test_dedupe_host.py for the crafted scenes, `_held_to_restatement` here for the others):
every D is at least 1e-9 (relative) away from max_dist, far more than the device's contraction of multiply-adds can move it.

The net-level tests run on the 200 x 264 synthetic ResNet-152 of tests/test_gpu_complete.py (maps of 25 x 33 cells), DC_AUTOTUNE=0."""
import numpy as np
import pytest

import complete_ref as D
import dedupe_ref as E
import dedupe_scenes as S
import people_ref as R
from conftest import rand_image

pytestmark = pytest.mark.gpu

H, W = 200, 264
EDGES = R.all_pairs_edges()
MEAN, STD = D.MEAN, D.STD
REAL = dict(threshold=0.5, radius=1, max_det=8, max_cost=40.0, seed_threshold=0.55, max_people=32, min_joints=2)
REAL_FILL = dict(fill_threshold=0.6, fill_radius=3, min_support=3)
_nets = {}


@pytest.fixture(scope="module", autouse=True)
def cost_model_tiles(gpu_caffe):
    """DC_AUTOTUNE=0 for every forward of the module: nothing is timed, and every executor of a model runs the same tiles."""
    import os

    old = os.environ.get("DC_AUTOTUNE")
    os.environ["DC_AUTOTUNE"] = "0"
    gpu_caffe.set_mode_gpu()
    yield
    if old is None:
        del os.environ["DC_AUTOTUNE"]
    else:
        os.environ["DC_AUTOTUNE"] = old
    _nets.clear()


# ---- the stage alone: dc_dedupe_people on crafted host arrays, scenes (a) to (g) ---------------------------------------------------
def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_crafted_scene_equals_the_restatement(gpu_caffe, name):
    sc = S.scene(name)
    n_out, people, cand, kept_from, by, _ = S.reference(name)
    got = gpu_caffe.dedupe_people(sc["people"], sc["n"], sc["cand"], dedupe=sc["params"], return_maps=True)
    assert len(got) == len(sc["n"])
    for b, g in enumerate(got):
        m, n = int(n_out[b]), int(sc["n"][b])
        assert g["people"].shape[0] == m and g["kept_from"].tolist() == sc["kept"][b] == kept_from[b, :m].tolist()
        assert _same_bytes(g["people"], people[b, :m]) and _same_bytes(g["cand"], cand[b, :m])
        assert _same_bytes(g["suppressed_by"], by[b, :n])


def test_the_padding_of_the_raw_call(gpu_caffe):
    """Beyond n_out: (0, 0, 0), cand -1, kept_from -1; beyond n_people: suppressed_by -1 — whatever the arrays held before."""
    import ctypes as C

    import caffe.pycaffe as pc

    sc = S.scene("e_batch_j32")
    n_out, people, cand, kept_from, by, _ = S.reference("e_batch_j32")
    q, _keep = pc._dedupe_struct(pc.dedupe_params(sc["params"]))
    nb, P, J = sc["people"].shape[:3]
    o_n, o_p, o_c = np.full(nb, 77, np.int32), np.full((nb, P, J, 3), 7.0), np.full((nb, P, J), 77, np.int32)
    o_f, o_b = np.full((nb, P), 77, np.int32), np.full((nb, P), 77, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert pc._lib.dc_dedupe_people(C.byref(q), nb, P, J, ptr(sc["n"]), ptr(sc["people"]), None, ptr(o_n), ptr(o_p), ptr(o_c), ptr(o_f),
                                    ptr(o_b)) == 0
    assert np.array_equal(o_n, n_out) and _same_bytes(o_p, people) and np.array_equal(o_c, cand)
    assert np.array_equal(o_f, kept_from) and np.array_equal(o_b, by)
    # the optional outputs left out
    o_p2 = np.full((nb, P, J, 3), 7.0)
    assert pc._lib.dc_dedupe_people(C.byref(q), nb, P, J, ptr(sc["n"]), ptr(sc["people"]), None, ptr(o_n), ptr(o_p2), None, None, None) == 0
    assert _same_bytes(o_p2, people)


def test_three_calls_one_result(gpu_caffe):
    sc = S.scene("d_words")
    runs = [gpu_caffe.dedupe_people(sc["people"], sc["n"], dedupe=sc["params"], return_maps=True)[0] for _ in range(3)]
    assert all(_same_bytes(r[k], runs[0][k]) for r in runs[1:] for k in runs[0])


# ---- through the nets ------------------------------------------------------------------------------------------------------------------
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


def _held_to_restatement(label, base, got, dd, least=1e-9):
    """base / got: an entry's results (lists of dicts) without and with dedupe.  Every image of `got` must be the restatement applied to
    that image of `base`, byte for byte, and every decision of the restatement at least `least` away from max_dist.
    -> (people before, people suppressed)."""
    assert len(base) == len(got)
    before = gone = 0
    worst = float("inf")
    for b, (x, y) in enumerate(zip(base, got)):
        ref = E.dedupe_ref(x["people"], x["cand"], **dd)
        worst = min(worst, E.check_margins(ref, dd["max_dist"], dd["min_common"], least=least))
        assert _same_bytes(y["people"], ref["people"]) and _same_bytes(y["cand"], ref["cand"]), (label, b)
        if "filled" in x:
            assert np.array_equal(y["filled"], y["cand"] == -2)
        before, gone = before + len(x["people"]), gone + len(x["people"]) - len(ref["people"])
    print("%s: %d people, %d suppressed, smallest margin %.3g" % (label, before, gone, worst))
    return before, gone


def fragment_scene(sixteen_bit=False):
    """The planted scene of tests/complete_ref.py with person 1 split by max_cost: every regression edge between its joints 0..6 and
    7..13, in both directions, predicts 24 px right of the truth, so those pair costs are 24 > max_cost = 20 and joints 7..13 seed a
    second person — while each fragment's predictors agree on where the other half is, 24 px right of it, and a dim peak (0.3125, below
    the assembly's threshold, three cells from the held peak and so outside its NMS radius) stands there for stage D to fill from."""
    sc = D.lowered_scene(sixteen_bit, lowered=())
    lut = R.edge_table(sc["edges"])
    q16 = R.round_to_bf16 if sixteen_bit else (lambda v: np.asarray(v, np.float32))
    for a in range(14):
        for c in range(14):
            if (a < 7) == (c < 7):
                continue
            l = lut[a, c]
            r, col = sc["cells"][1, a]
            _, nt = R.M.encode_targets(sc["joints"][1, a], sc["joints"][1, c] + [24.0, 0.0], (r, col), 1.0, MEAN[l], STD[l])
            sc["nxt"][2 * l:2 * l + 2, r, col] = q16(nt)
    for j in range(14):
        x, y = sc["joints"][1, j] + [24.0, 0.0]
        r, col = int(y // 8), int(x // 8)
        assert abs(col - sc["cells"][1, j][1]) >= 2 and sc["prob"][j, max(r - 1, 0):r + 2, col - 1:col + 2].max() == 0
        sc["prob"][j, r, col] = 0.3125
    return sc


FRAGMENT_DD = dict(max_dist=0.1, min_common=3, min_size=32.0, sigma=None, absorb=True)


def _fragments_through_the_chain(n, sixteen_bit):
    sc = fragment_scene(sixteen_bit)
    n.blobs["prob"].data[0], n.blobs["loc_pred"].data[0], n.blobs["next_pred"].data[0] = sc["prob"], sc["loc"], sc["nxt"]
    n.blobs["prob"].data[1] = 0
    kw = dict(scale=1.0, edges=sc["edges"], mean=MEAN, std=STD, **D.ASSEMBLY)
    plain = n.assemble_people(**kw)
    # stage C alone: four people, the human in the middle as two halves with no joint in common
    assert len(plain[0]["cand"]) == 4 and len(plain[1]["cand"]) == 0
    halves = [q for q in range(4) if (plain[0]["cand"][q] >= 0).sum() == 7]
    assert len(halves) == 2 and not ((plain[0]["cand"][halves[0]] >= 0) & (plain[0]["cand"][halves[1]] >= 0)).any()
    base = n.assemble_people(complete=D.FILL, **kw)
    assert len(base[0]["cand"]) == 4 and (base[0]["cand"][halves] == -2).sum() == 14  # stage D: both are full skeletons now
    got = n.assemble_people(complete=D.FILL, dedupe=FRAGMENT_DD, **kw)
    assert n.dedupe is None and n.completion is None
    before, gone = _held_to_restatement("fragments", base, got, FRAGMENT_DD)
    assert (before, gone) == (4, 1) and len(got[0]["cand"]) == 3 and len(got[1]["cand"]) == 0
    # the survivor is the human again: fourteen joints of stage C, at the planted points
    one = got[0]["cand"][halves[0]]
    assert (one >= 0).all() and not got[0]["filled"][halves[0]].any()
    assert np.abs(got[0]["people"][halves[0], :, :2] - sc["joints"][1]).max() <= (0.5 if sixteen_bit else 1e-9)
    # without absorb the better half stays as stage D left it
    keep = n.assemble_people(complete=D.FILL, dedupe=dict(FRAGMENT_DD, absorb=False), **kw)
    _held_to_restatement("fragments, no absorb", base, keep, dict(FRAGMENT_DD, absorb=False))
    assert _same_bytes(keep[0]["people"][halves[0]], base[0]["people"][halves[0]]) and (keep[0]["cand"][halves[0]] == -2).sum() == 7
    return kw, base, got


def test_fragments_whole_chain(planted):
    """(h) max_cost splits one human in two, completion turns the halves into doubles, dedupe leaves one — with the stage-C joints of
    both.  As an argument and as the net's setting; three calls, one result."""
    kw, base, got = _fragments_through_the_chain(planted, False)
    planted.dedupe, planted.completion = FRAGMENT_DD, D.FILL
    try:
        for _ in range(2):
            again = planted.assemble_people(**kw)
            assert all(_same_bytes(x[k], y[k]) for x, y in zip(again, got) for k in ("people", "cand", "filled"))
        off_once = planted.assemble_people(dedupe=False, **kw)
        assert planted.dedupe is not None
    finally:
        planted.dedupe = planted.completion = None
    assert all(_same_bytes(x[k], y[k]) for x, y in zip(off_once, base) for k in ("people", "cand", "filled"))


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_fragments_on_sixteen_bit_nets(gpu_caffe, synth152, dtype):
    n = _net("planted:" + dtype, gpu_caffe, synth152[0])
    assert n.dtype == dtype
    _fragments_through_the_chain(n, True)


def _same_result(a, b, keys=("people", "cand", "cost")):
    return len(a) == len(b) and all(_same_bytes(x[k], y[k]) for x, y in zip(a, b) for k in keys)


def test_off_is_off(gpu_caffe, synth152):
    """(i) A net that never had dedupe set, the same net with it set, and with it unset again: the first and the third call give the
    same bits in people, cand and cost.  Set with max_dist = 0 on distinct poses: the launch runs and the people are the same."""
    from deepcut_tools import deepercut_prototxt

    fresh = gpu_caffe.Net(deepercut_prototxt(152, H, W), synth152[0], gpu_caffe.TEST, from_text=True)
    fresh.forward_batch(rand_image(12, H, W, n=2), want=())
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, return_cost=True, **REAL)
    first = fresh.assemble_people(**kw)
    assert fresh.dedupe is None and sum(len(d["cand"]) for d in first) > 2
    fresh.dedupe = dict(max_dist=1e6, min_common=1)
    merged = fresh.assemble_people(**kw)
    assert sum(len(d["cand"]) for d in merged) < sum(len(d["cand"]) for d in first)
    fresh.dedupe = None
    third = fresh.assemble_people(**kw)
    assert _same_result(first, third) and _same_result(fresh.assemble_people(dedupe=None, **kw), first)
    # distinct poses, max_dist 0: nobody is anybody else
    for d in first:
        assert all(D_ > 0 for D_ in E.all_distances(d["people"], 1, 32.0))
    zero = fresh.assemble_people(dedupe=dict(max_dist=0.0, min_common=1, absorb=True), **kw)
    assert _same_result(zero, first)


def _pick(base, min_common=3, min_size=32.0, absorb=True, sigma=None):
    """max_dist for a real forward: the midpoint of the widest gap between consecutive sorted D values (all images pooled) whose lower
    end lies between the 10th and the 40th percentile.  Half that gap must be >= 1e-9 max_dist."""
    Ds = sorted(v for d in base for v in E.all_distances(d["people"], min_common, min_size, sigma) if np.isfinite(v))
    assert len(Ds) >= 10, len(Ds)
    lo, hi = int(np.ceil(0.1 * (len(Ds) - 1))), int(np.floor(0.4 * (len(Ds) - 1)))
    i = max(range(lo, hi + 1), key=lambda k: Ds[k + 1] - Ds[k])
    md = 0.5 * (Ds[i] + Ds[i + 1])
    assert 0.5 * (Ds[i + 1] - Ds[i]) >= 1e-9 * md, (Ds[i], Ds[i + 1])
    return dict(max_dist=md, min_common=min_common, min_size=min_size, sigma=sigma, absorb=absorb)


def test_real_forward_batch_two(real):
    """(j) Random maps of the synthetic net, batch 2, completion on so that people share joints.  Three identical calls, one result."""
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, complete=REAL_FILL, **REAL)
    base = real.assemble_people(**kw)
    dd = _pick(base)
    runs = [real.assemble_people(dedupe=dd, **kw) for _ in range(3)]
    assert _same_result(runs[0], runs[1], ("people", "cand", "filled")) and _same_result(runs[0], runs[2], ("people", "cand", "filled"))
    before, gone = _held_to_restatement("real forward", base, runs[0], dd)
    assert gone >= 1 and before - gone >= 1  # a condition on the seed of the images: the restatement both suppresses and keeps
    # a sigma per joint and no absorb
    dd2 = _pick(base, min_common=2, min_size=64.0, absorb=False, sigma=[0.5 + (j % 4) / 4.0 for j in range(14)])
    _held_to_restatement("real forward, sigma", base, real.assemble_people(dedupe=dd2, **kw), dd2)
    # what only the joints decide is refused by the assembling call
    import caffe

    for bad in (dict(sigma=[1.0] * 13), dict(min_common=15)):
        with pytest.raises(caffe.DeepcutError) as ei:
            real.assemble_people(dedupe=dict(dd, **bad), **kw)
        assert ei.value.code == -3 and real.dedupe is None


def test_sparse_pairwise(gpu_caffe, synth152):
    """(k) A net narrowed to loc_pred and prob with the sparse pairwise head."""
    n = _net("sparse", gpu_caffe, synth152[0])
    assert n.wanted_outputs == ["loc_pred", "prob"] and n.sparse_pairwise
    kw = dict(scale=1.0, edges=EDGES, mean=MEAN, std=STD, complete=REAL_FILL, **REAL)
    base = n.assemble_people(**kw)
    dd = _pick(base)
    before, gone = _held_to_restatement("sparse pairwise", base, n.assemble_people(dedupe=dd, **kw), dd)
    assert gone >= 1


@pytest.mark.parametrize("flip", [False, True], ids=["pyramid", "pyramid_and_mirror"])
def test_fused_pyramid_and_mirror(gpu_caffe, synth152, flip):
    """(k) NetGroup.assemble_people on two scales, and on the same two with their mirrors, through the group's own setting; a member's
    setting is not read."""
    from deepcut_tools import deepercut_prototxt
    from pose.people import MIRROR_MPII14

    img = np.random.RandomState(37).randint(0, 256, (2, H, W, 3)).astype(np.uint8)
    scales = (1.0, 0.7, 1.0, 0.7) if flip else (1.0, 0.7)
    mkw = dict(mirror=(0, 0, 1, 1), image_width=W, joint_mirror=MIRROR_MPII14) if flip else {}
    shapes = [(2,) + tuple(gpu_caffe.canvas_size(H, W, s)) for s in scales]
    net = gpu_caffe.Net(deepercut_prototxt(152, shapes[0][1], shapes[0][2], 2), synth152[0], gpu_caffe.TEST, from_text=True)
    grp = gpu_caffe.NetGroup.for_shapes(net, shapes)
    grp.forward_images(img, scales, want=(), pose=False, mirror=mkw.get("mirror"))
    kw = dict(edges=EDGES, mean=MEAN, std=STD, complete=REAL_FILL, **dict(REAL, **mkw))
    base = grp.assemble_people(scales, 0, **kw)
    dd = _pick(base)
    grp.nets[0].dedupe = dict(max_dist=1e6, min_common=1)  # not read
    assert _same_result(grp.assemble_people(scales, 0, **kw), base, ("people", "cand", "filled"))
    grp.dedupe = dd
    got = grp.assemble_people(scales, 0, **kw)
    grp.dedupe = None
    before, gone = _held_to_restatement("fused " + ("pyramid + mirror" if flip else "pyramid"), base, got, dd)
    assert gone >= 1
    assert _same_result(grp.assemble_people(scales, 0, dedupe=dd, **kw), got, ("people", "cand", "filled")) and grp.dedupe is None
    assert _same_result(grp.assemble_people(scales, 0, **kw), base, ("people", "cand", "filled"))


# ---- tracker, async entry, frames in flight --------------------------------------------------------------------------------------------
TKW = dict(max_misses=1, min_common=1, max_dist=4.0, min_size=16.0, motion=1)
IMG = np.random.RandomState(4).randint(0, 256, (H - 3, W - 5, 3)).astype(np.uint8)
FRAMES = [np.ascontiguousarray(np.roll(IMG, 8 * k, axis=1)) for k in range(4)]
CHAIN = dict(edges=EDGES, mean=MEAN, std=STD, threshold=0.5, max_det=8, max_cost=40.0, seed_threshold=0.55, min_joints=2, complete=REAL_FILL)


@pytest.fixture(scope="module")
def video_net(gpu_caffe, synth152):
    from deepcut_tools import deepercut_prototxt

    return gpu_caffe.Net(deepercut_prototxt(152, H, W), synth152[0], gpu_caffe.TEST, from_text=True)


def _frame_dd(net, frame):
    net.forward_images(frame, 1.0, want=(), pose=False)
    base = net.assemble_people(scale=1.0, **CHAIN)
    return base, _pick(base)


def test_the_tracker_sees_the_people_that_were_kept(video_net, gpu_caffe):
    """(k) track_people(dedupe=...) returns assemble_people(dedupe=...)'s people bit for bit; its ids are those Tracker.update gives on
    these people; the tracker holds one track per survivor, and a second identical frame matches exactly those."""
    net = video_net
    base, dd = _frame_dd(net, FRAMES[0])
    chained, by_hand = gpu_caffe.Tracker(n_joints=14, **TKW), gpu_caffe.Tracker(n_joints=14, **TKW)
    want = net.assemble_people(scale=1.0, dedupe=dd, **CHAIN)
    before, gone = _held_to_restatement("tracked frame", base, want, dd)
    assert gone >= 1
    m = before - gone
    for k in range(2):  # the frame, and the same frame again
        got = net.track_people(chained, scale=1.0, dedupe=dd, **CHAIN)[0]
        assert all(_same_bytes(got[key], want[0][key]) for key in ("people", "cand", "filled"))
        ids, place = by_hand.update([want[0]["people"]])
        assert np.array_equal(ids[0, :m], got["ids"]) and np.array_equal(place[0, :m], got["place"])
        assert sorted(got["ids"].tolist()) == list(range(m))  # births in the first frame, the same ids in the second
    st = chained.state()
    assert (st["ids"] >= 0).sum() == m and (st["hits"][st["ids"] >= 0] == 2).all()
    # the cleaned top-down way gives the same people: the stage alone on the entry's own output
    alone = gpu_caffe.dedupe_people([base[0]["people"]], cand=[base[0]["cand"]], dedupe=dd)[0]
    assert _same_bytes(alone["people"], want[0]["people"]) and _same_bytes(alone["cand"], want[0]["cand"])


def test_async_entry_and_frames_in_flight(video_net, gpu_caffe):
    """(k) track_frames_async(...).result() and a VideoPipeline of depth 2 give what the synchronous loop gives, bit for bit, with
    dedupe on: as an argument of every request, and as the net's setting, which the pipeline's clone copies."""
    from deepcut_tools import VideoPipeline

    net = video_net
    base, dd = _frame_dd(net, FRAMES[0])
    by_hand = gpu_caffe.Tracker(n_joints=14, **TKW)
    want = []
    for f in FRAMES:
        net.forward_images(f, 1.0, want=(), pose=False)
        want.append(net.track_people(by_hand, scale=1.0, dedupe=dd, **CHAIN)[0])
    assert _same_bytes(want[0]["people"], E.dedupe_ref(base[0]["people"], base[0]["cand"], **dd)["people"])
    assert len(want[0]["people"]) < len(base[0]["people"]) and net.dedupe is None
    keys = ("people", "cand", "filled", "ids", "place")
    tracker = gpu_caffe.Tracker(n_joints=14, **TKW)
    got = [net.track_frames_async(f, tracker, 1.0, dedupe=dd, **CHAIN).result()[0] for f in FRAMES]
    assert all(_same_bytes(g[k], w[k]) for g, w in zip(got, want) for k in keys) and net.dedupe is None
    a, b = tracker.state(), by_hand.state()
    assert all(np.array_equal(a[k], b[k]) for k in a)
    for as_state in (False, True):
        tracker = gpu_caffe.Tracker(n_joints=14, **TKW)
        net.dedupe = dd if as_state else None
        pipe = VideoPipeline(net, tracker, depth=2, stats=(EDGES, MEAN, STD), choose_streams=False, dedupe=None if as_state else dd,
                             **{k: v for k, v in CHAIN.items() if k not in ("edges", "mean", "std")})
        assert [m.dedupe is not None for m in pipe.nets] == [as_state] * 2
        for k, f in enumerate(FRAMES):
            pipe.submit(f, tag=k)
        out = pipe.drain()
        net.dedupe = None
        assert [t for t, _, _ in out] == list(range(len(FRAMES)))
        for (_, people, ids), w in zip(out, want):
            assert _same_bytes(people, w["people"]) and np.array_equal(ids, w["ids"])

"""CPU: the host side of the skeleton overlay (include/deepcut_hip.h, dc_draw_people) — the restatement's guarded int64 coverage against
exact integer arithmetic, the forward colour rule's coefficient integers and its round trip through the existing inverse rule over all
2^24 R, G, B triples, every refusal of the entry without a device, and the `draw=` switch of VideoPipeline / track_people on a fake net.

PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host; the rule is this project's own.

The round-trip bounds (2 levels limited range, 1 level full range) are the ones the rule's statement gives: a limited-range triple is
quantised to 219 / 224 levels on the way forward, so one level of Y, Cb or Cr is up to 255/219 * 1 or 255/224 * 1.772 > 1 level of R, G, B."""
import ctypes as C

import numpy as np
import pytest

import draw_ref as DR
import nv12_ref as NR
from test_video_host import STATS, FakeNet, _frame

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
TABLE = {
    ("bt601", "limited"): ((16829, 33039, 6416), (-9714, -19071, 28784), (28784, -24103, -4681), 16),
    ("bt601", "full"): ((19595, 38470, 7471), (-11058, -21710, 32768), (32768, -27439, -5329), 0),
    ("bt709", "limited"): ((11966, 40254, 4064), (-6596, -22189, 28784), (28784, -26145, -2639), 16),
    ("bt709", "full"): ((13933, 46871, 4732), (-7509, -25259, 32768), (32768, -29763, -3005), 0),
}


def test_guarded_coverage_equals_exact_integer_arithmetic():
    """64 x 256 frame, seeded segments; a third of them tens of thousands of pixels long through the frame, some clamped."""
    H, W = 64, 256
    rs = np.random.RandomState(11)
    guard = tests = 0
    for i in range(36):
        r16 = int(rs.randint(1, 1025))
        if i % 3 == 0:  # through a point of the frame, the ends 8 000 .. 40 000 px away on either side (beyond the clamp at times)
            c = np.array([rs.uniform(0, W), rs.uniform(0, H)])
            t = rs.uniform(0, 2 * np.pi)
            u = np.array([np.cos(t), np.sin(t)])
            a, b = c - u * rs.uniform(8000, 40000), c + u * rs.uniform(8000, 40000)
        else:
            a = np.array([rs.uniform(-40, W + 40), rs.uniform(-40, H + 40)])
            b = a + rs.uniform(-120, 120, 2)
        qa, qb = (DR.snap(a[0]), DR.snap(a[1])), (DR.snap(b[0]), DR.snap(b[1]))
        assert max(abs(v) for v in qa + qb) <= 1 << 19
        got, g = DR.coverage(H, W, qa, qb, r16, True)
        assert np.array_equal(got, DR.coverage_exact(H, W, qa, qb, r16, True)), (i, qa, qb, r16)
        disc, _ = DR.coverage(H, W, qa, qa, r16, False)
        assert np.array_equal(disc, DR.coverage_exact(H, W, qa, qa, r16, False))
        guard, tests = guard + g, tests + H * W
    print("%d pixel tests, %d took the guard" % (tests, guard))
    assert guard >= 1


def test_snap_is_ties_to_even_and_clamped():
    assert [DR.snap(v) for v in (0.03125, 0.09375, -0.03125, 1.0, 1e9, -1e9, 32768.5)] == [0, 2, 0, 16, 1 << 19, -(1 << 19), 1 << 19]


@pytest.mark.parametrize("pair", sorted(TABLE))
def test_forward_coefficients_are_the_table(pair):
    import caffe

    assert caffe.draw_coefficients(*pair) == TABLE[pair]
    assert DR.forward_coefficients(*pair) == TABLE[pair]


@pytest.mark.parametrize("pair", sorted(TABLE))
def test_forward_then_inverse_comes_back_on_all_triples(pair):
    matrix, range_ = pair
    bound = 2 if range_ == "limited" else 1
    worst = 0
    g, b = np.meshgrid(np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32), indexing="ij")
    g, b = g.ravel(), b.ravel()
    for r0 in range(0, 256, 32):
        for r in range(r0, r0 + 32):
            R = np.full_like(g, r)
            Y, Cb, Cr = DR.forward(R, g, b, matrix, range_)
            if range_ == "limited":
                assert Y.min() >= 16 and Y.max() <= 235 and min(Cb.min(), Cr.min()) >= 16 and max(Cb.max(), Cr.max()) <= 240
            back = NR.convert(Y, Cb, Cr, matrix, range_)
            worst = max(worst, max(int(np.abs(v - w).max()) for v, w in zip(back, (R, g, b))))
    print("%s %s: max |inverse(forward(rgb)) - rgb| = %d level(s) over 2^24 triples" % (matrix, range_, worst))
    assert worst <= bound


# ---- the entry's refusals, without a device -------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_mode():
    import caffe
    import caffe.pycaffe as pc

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield caffe, pc
    pc._lib.dc_set_mode(mode)


def _raw(pc, H=20, W=30, fmt=1, nb=2, P=4, J=14, frames=None, n_people=None, **style):
    """dc_draw_people through ctypes with good arguments except what the caller overrides -> (rc, message)."""
    y, uv = np.zeros((H, W), np.uint8), np.zeros(((H + 1) // 2, (W + 1) // 2, 2), np.uint8)
    bgr = np.zeros((H, W, 3), np.uint8)
    arr = (pc.DcFrame * max(nb, 1))()
    for f in arr:
        if fmt == 0:
            f.plane[0], f.pitch[0] = bgr.ctypes.data, 3 * W
        else:
            f.plane[0], f.plane[1], f.pitch[0], f.pitch[1] = y.ctypes.data, uv.ctypes.data, W, 2 * ((W + 1) // 2)
        f.format = fmt
    if frames:
        frames(arr)
    n = np.ascontiguousarray([1] * max(nb, 1) if n_people is None else n_people, np.int32)
    people = np.ones((max(nb, 1), max(P, 1), max(J, 1), 3))
    given = style.pop("edges", [(0, 1), (1, 2)])
    edges = np.ascontiguousarray([] if given is None else given, np.int32).reshape(-1, 2)
    pal = np.ascontiguousarray([(255, 0, 0), (0, 255, 0)], np.uint8)
    st = pc.DrawStyle()
    st.n_edges, st.edges = style.pop("n_edges", edges.shape[0]), None if given is None else edges.ctypes.data
    st.joint_radius, st.limb_radius, st.alpha, st.alpha_filled, st.min_score = 4.0, 2.0, 256, 128, 0.0
    st.color_mode, st.palette, st.n_palette = 0, pal.ctypes.data, 2
    for k, v in style.items():
        setattr(st, k, v)
    rc = pc._lib.dc_draw_people(arr, nb, H, W, 0, P, J, n.ctypes.data_as(C.c_void_p), people.ctypes.data_as(C.c_void_p), None, None, C.byref(st),
                                None)
    return rc, (pc._lib.dc_last_error() or b"").decode()


def test_every_argument_error_is_einval_naming_the_field(cpu_mode):
    _caffe, pc = cpu_mode

    def frame1(field, value, k=None):
        def change(arr):
            if k is None:
                setattr(arr[1], field, value)
            else:
                getattr(arr[1], field)[k] = value
        return change

    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(frames=frame1("plane", None, 1)), ("frame 1", "plane[1]")),
        (dict(frames=frame1("plane", None, 0), fmt=0), ("frame 1", "plane[0]")),
        (dict(frames=frame1("pitch", 29, 0)), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("pitch", 28, 1)), ("frame 1", "pitch[1]")),
        (dict(frames=frame1("pitch", 89, 0), fmt=0), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("format", 7)), ("frame 1", "format")),
        (dict(frames=frame1("matrix", 2)), ("frame 1", "matrix")),
        (dict(frames=frame1("range", -1)), ("frame 1", "range")),
        (dict(frames=frame1("format", 0)), ("frame 1", "format", "differs")),
        (dict(frames=frame1("matrix", 1)), ("frame 1", "matrix", "differs")),
        (dict(frames=frame1("range", 1)), ("frame 1", "range", "differs")),
        (dict(nb=0), ("nb",)), (dict(nb=65), ("nb",)),
        (dict(P=0), ("P",)), (dict(P=257), ("P",)), (dict(J=0), ("J",)), (dict(J=33), ("J",)),
        (dict(W=16385), ("width",)), (dict(H=16385, W=1), ("height",)),
        (dict(joint_radius=-0.5), ("joint_radius",)), (dict(joint_radius=64.5), ("joint_radius",)), (dict(joint_radius=nan), ("joint_radius",)),
        (dict(limb_radius=-1.0), ("limb_radius",)), (dict(limb_radius=65.0), ("limb_radius",)), (dict(limb_radius=inf), ("limb_radius",)),
        (dict(alpha=-1), ("alpha",)), (dict(alpha=257), ("alpha",)),
        (dict(alpha_filled=-1), ("alpha_filled",)), (dict(alpha_filled=257), ("alpha_filled",)),
        (dict(min_score=-0.1), ("min_score",)), (dict(min_score=nan), ("min_score",)), (dict(min_score=inf), ("min_score",)),
        (dict(color_mode=2), ("color_mode",)), (dict(color_mode=-1), ("color_mode",)),
        (dict(palette=None), ("palette",)), (dict(n_palette=0), ("n_palette",)), (dict(n_palette=257), ("n_palette",)),
        (dict(n_edges=-1), ("n_edges",)), (dict(n_edges=129), ("n_edges",)), (dict(edges=None, n_edges=2), ("edges",)),
        (dict(edges=[(0, 1), (3, 14)]), ("edges[1]", "14")), (dict(edges=[(-1, 1)]), ("edges[0]", "-1")), (dict(edges=[(0, 1), (2, 3)], J=3), ("edges[1]",)),
        (dict(n_people=[1, 5]), ("n_people[1]",)), (dict(n_people=[-1, 0]), ("n_people[0]",)),
    ]
    for kw, words in cases:
        rc, msg = _raw(pc, **kw)
        assert rc == EINVAL and "draw_people" in msg and all(w in msg for w in words), (kw, rc, msg)
    # good arguments, both formats, joints only, the limits themselves: there is no CPU path
    for kw in (dict(), dict(fmt=0), dict(n_edges=0), dict(nb=64, P=256, J=32), dict(alpha=0, alpha_filled=256, joint_radius=0.0, limb_radius=64.0),
               dict(n_people=[0, 0])):
        rc, msg = _raw(pc, **kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)
    # NULL arguments
    assert pc._lib.dc_draw_people(None, 1, 4, 4, 0, 1, 1, None, None, None, None, None, None) == EINVAL
    t = [C.c_int() for _ in range(3)]
    assert pc._lib.dc_draw_limits(C.byref(t[0]), C.byref(t[1]), None) == 0 and t[0].value > 0 and t[0].value % 2 == 0 and t[1].value % 2 == 0


def test_python_entry_refusals(cpu_mode):
    caffe, _pc = cpu_mode
    people = np.ones((2, 14, 3))
    img = np.zeros((20, 30, 3), np.uint8)
    frozen = img.copy()
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="writable"):
        caffe.draw_people(frozen, people)
    y, uv = np.zeros((20, 30), np.uint8), np.zeros((10, 15, 2), np.uint8)
    uv.flags.writeable = False
    with pytest.raises(ValueError, match="writable"):
        caffe.draw_people(caffe.Frame.nv12(y, uv), people)
    with pytest.raises(ValueError, match="frames"):
        caffe.draw_people("picture", people)
    with pytest.raises(ValueError, match="color"):
        caffe.draw_people(img, people, color="rainbow")
    with pytest.raises(ValueError, match="one entry per frame"):
        caffe.draw_people(img, np.ones((2, 3, 14, 3)))
    with pytest.raises(ValueError, match="ids"):
        caffe.draw_people(img, people, ids=[1, 2, 3])
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.draw_people(img, people, edges=[(0, 14)])
    assert ei.value.code == EINVAL and "edges[0]" in str(ei.value)
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.draw_people(img, people, alpha=300)
    assert ei.value.code == EINVAL and "alpha" in str(ei.value)
    import pose

    for call in (lambda: caffe.draw_people(img, people, ids=[3, -1], cand=np.full((2, 14), -2, np.int32)),
                 lambda: caffe.draw_people([caffe.Frame.bgr(img), caffe.Frame.bgr(img.copy())], [people, people[:0]], color="joint"),
                 lambda: pose.draw_people(img, people, ids=np.array([0, 1]))):
        with pytest.raises(caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == ENOCPU
    assert not img.any()
    assert len(pose.SKELETON_MPII14) == 14 and all(0 <= a < 14 and 0 <= c < 14 for a, c in pose.SKELETON_MPII14)
    # the skeleton is its own mirror image under the joint mirror table: left and right limbs are drawn alike
    mirrored = set(tuple(sorted((pose.MIRROR_MPII14[a], pose.MIRROR_MPII14[c]))) for a, c in pose.SKELETON_MPII14)
    assert mirrored == set(tuple(sorted(e)) for e in pose.SKELETON_MPII14)
    assert len(caffe.DRAW_JOINT_COLORS) == 14 and len(caffe.DRAW_ID_COLORS) >= 1 and caffe.draw_limits()[2] >= 1


# ---- draw= of the pipeline and of track_people on a fake net --------------------------------------------------------------------------
def test_draw_none_never_touches_the_draw_entry(monkeypatch):
    """With the entry REMOVED from every module that offers it, the default runs as before: no attribute access, no call."""
    import caffe
    import caffe.pycaffe as pc
    import pose
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    for mod in (caffe, pc, pose, pp):
        monkeypatch.delattr(mod, "draw_people")
    monkeypatch.delattr(pp, "_draw_style")
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=2, stats=STATS, choose_streams=False)
    for k in range(5):
        pipe.submit(_frame(k), tag=k)
    assert [t for t, _, _ in pipe.drain()] == list(range(5))
    monkeypatch.undo()
    for mod in (caffe, pc, pose, pp):
        monkeypatch.delattr(mod, "draw_people")
    net = FakeNet()
    out = list(pose.track_people([_frame(k) for k in range(3)], None, None, STATS, tracker="tracker", depth=1, batch=2, net=net))
    assert [int(p[0, 0, 0]) for p, _ in out] == [0, 1, 2] and all("draw" not in c["kw"] for c in net.world["calls"])


def test_draw_keeps_each_frame_with_its_request_and_draws_before_handing_back(monkeypatch):
    import pose.people as pp
    from deepcut_tools import VideoPipeline

    drawn = []
    monkeypatch.setattr(pp, "draw_people", lambda frame, people, ids=None, **style: drawn.append((frame, people, ids, style)))
    net = FakeNet()
    pipe = VideoPipeline(net, "tracker", depth=2, batch=2, stats=STATS, choose_streams=False, draw=dict(alpha=96))
    frames = [_frame(k) for k in range(5)]
    for k, f in enumerate(frames):
        pipe.submit(f, tag=k)
    assert all("draw" not in c["kw"] for c in net.world["calls"])  # the style stays with the pipeline
    tag, people, ids = pipe.wait_one()
    assert tag == 0 and len(drawn) == 2 and drawn[0][0] is frames[0] and drawn[0][1] is people and drawn[0][2] is ids  # its batch was drawn
    out = [(tag, people, ids)] + pipe.drain()
    assert len(drawn) == 5 and all(d[0] is f for d, f in zip(drawn, frames)) and all(d[1] is o[1] and d[3] == dict(alpha=96, cand=None) for d, o in zip(drawn, out))
    with pytest.raises(ValueError, match="draw"):
        VideoPipeline(FakeNet(), "tracker", stats=STATS, draw="yes")
    # track_people hands the style on, (people, ids) are what they are without it
    drawn[:] = []
    plain = list(pp.track_people([_frame(k) for k in range(3)], None, None, STATS, tracker="tracker", depth=1, batch=2, net=FakeNet()))
    frames = [_frame(k) for k in range(3)]
    with_draw = list(pp.track_people(frames, None, None, STATS, tracker="tracker", depth=1, batch=2, net=FakeNet(), draw=True))
    assert len(drawn) == 3 and all(d[0] is f for d, f in zip(drawn, frames)) and all(d[3] == dict(cand=None) for d in drawn)
    for (p0, i0), (p1, i1) in zip(plain, with_draw):
        assert np.array_equal(p0, p1) and np.array_equal(i0, i1)

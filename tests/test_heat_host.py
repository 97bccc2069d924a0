"""CPU: the host side of the score-map overlay (include/deepcut_hip.h, dc_draw_heatmap) — properties of the numpy restatement
tests/heat_ref.py that follow from the rule's statement, every refusal of the three entries without a device, and DC_ENOCPU behind them.

PARITY UNPINNED BY THE REFERENCE: its demo draws 14 numpy circles and never shows a map; the rule is this project's own."""
import ctypes as C

import numpy as np
import pytest

import heat_ref as HR

EINVAL, ENOCPU = -1, -6  # include/deepcut_hip.h
LUT = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)  # every entry distinct
PAL = ((255, 0, 0), (0, 255, 0), (0, 0, 255))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_a_map_of_ones_at_full_alpha_is_the_luts_last_colour_everywhere():
    img = np.random.RandomState(1).randint(0, 256, (37, 45, 3)).astype(np.uint8)
    HR.draw_bgr(img, np.ones((3, 5, 6), np.float32), 1.37, mode="max", alpha=256, alpha_mode="const", lut=LUT)
    assert (img == LUT[255][::-1]).all()
    y, uv = np.zeros((37, 45), np.uint8), np.zeros((19, 23, 2), np.uint8)
    HR.draw_nv12(y, uv, np.ones((3, 5, 6), np.float32), 1.37, mode="max", alpha=256, alpha_mode="const", lut=LUT)
    Y, Cb, Cr = HR.DR.forward(*[int(v) for v in LUT[255]], "bt601", "limited")
    assert (y == Y).all() and (uv[:, :, 0] == Cb).all() and (uv[:, :, 1] == Cr).all()


@pytest.mark.parametrize("mode", ["max", "joints"])
def test_score_alpha_on_a_map_of_zeros_touches_nothing(mode):
    img = np.random.RandomState(2).randint(0, 256, (20, 30, 3)).astype(np.uint8)
    was = img.copy()
    scores = np.array([0.0, -0.0, -3.0, np.nan], np.float32).reshape(1, 2, 2).repeat(2, axis=0)
    HR.draw_bgr(img, scores, 1.0, mode=mode, alpha=256, alpha_mode="score", lut=LUT, palette=PAL)
    assert np.array_equal(img, was)
    assert all(not m.any() for m, _, _ in HR.layers(scores, *HR.luma_tables(20, 30, 2, 2, 1.0, (0, 0)), dict(mode=mode, alpha=256, alpha_mode="score")))


def test_quantisation_clamps_rounds_to_even_and_counts_nan_as_zero():
    s = np.array([np.nan, -0.0, -1.0, 2.0, np.inf, -np.inf, 1.0, 0.5, 0.5 / 4096, 1.5 / 4096, 2.5 / 4096, np.float32(1) - np.float32(2) ** -24])
    assert HR.quantise(s).tolist() == [0, 0, 0, 4096, 4096, 0, 4096, 2048, 0, 2, 2, 4096]
    assert HR.quantise(np.float16(0.3333)).item() == int(np.rint(np.float32(np.float16(0.3333)) * np.float32(4096)))


def test_at_scale_one_pixel_8c_plus_4_sits_on_a_cell_centre():
    """With the origin at (0.5, 0.5) the centre of pixel x is x itself: pixel 8 c + 4 is cell c's centre, f == 0 and v == q."""
    hm, wm = 4, 5
    q = np.random.RandomState(3).randint(0, 4097, (hm, wm)).astype(np.int32)
    tx, ty = HR.luma_tables(8 * hm, 8 * wm, hm, wm, 1.0, (0.5, 0.5))
    cols, rows = 8 * np.arange(wm) + 4, 8 * np.arange(hm) + 4
    assert np.array_equal(tx[cols], 256 * np.arange(wm)) and np.array_equal(ty[rows], 256 * np.arange(hm))
    v = HR.interpolate(q, tx, ty)
    assert np.array_equal(v[np.ix_(rows, cols)], q)
    assert v.min() >= 0 and v.max() <= 4096
    # between two centres the steps are 1/8 cell = 32/256
    assert np.array_equal(tx[4:13], 32 * np.arange(9))


def test_clamping_at_all_four_borders():
    """A frame that overhangs the map on every side: the overhang takes the border cells' values, never a cell outside."""
    hm, wm = 3, 4
    q = (np.arange(hm * wm, dtype=np.int32).reshape(hm, wm) + 1) * 300
    tx, ty = HR.luma_tables(8 * hm + 40, 8 * wm + 40, hm, wm, 1.0, (20.0, 20.0))
    assert tx.min() == 0 and tx.max() == 256 * (wm - 1) and ty.min() == 0 and ty.max() == 256 * (hm - 1)
    v = HR.interpolate(q, tx, ty)
    assert (v[:20, :20] == q[0, 0]).all() and (v[:20, -20:] == q[0, -1]).all() and (v[-20:, :20] == q[-1, 0]).all() and (v[-20:, -20:] == q[-1, -1]).all()
    # the last cell has no right / lower neighbour: i1 == i0 there, and f == 0
    assert (tx[-20:] & 255 == 0).all() and (ty[-20:] & 255 == 0).all()
    # the whole map off-frame to one side: everything clamps to one column
    tx, _ = HR.luma_tables(8, 45, hm, wm, 1.0, (-1000.0, 0.0))
    assert (tx == 256 * (wm - 1)).all()
    tx, _ = HR.luma_tables(8, 45, hm, wm, 1.0, (1000.0, 0.0))
    assert (tx == 0).all()


def test_ties_go_to_even_at_scale_one_sixtyfourth():
    """scale 1/64, origin -255.5: 256 u = x / 2 exactly, so odd x are exact halves."""
    tx, _ = HR.luma_tables(1, 12, 2, 6, 1.0 / 64.0, (-255.5, 0.0))
    assert tx.tolist() == [0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 5, 6]


@pytest.mark.parametrize("h,w", [(6, 8), (5, 7), (37, 45), (1, 1)])
def test_chroma_tables_use_block_centres_also_at_odd_sizes(h, w):
    hm, wm = 5, 6
    cx, cy = HR.chroma_tables(h, w, hm, wm, 1.0, (0.0, 0.0))
    assert len(cx) == (w + 1) // 2 and len(cy) == (h + 1) // 2
    # centre 2 b + 1: 256 u = 32 (2 b + 1 - 4), exact
    assert np.array_equal(cx, np.clip(32 * (2 * np.arange(len(cx)) - 3), 0, 256 * (wm - 1)))
    assert np.array_equal(cy, np.clip(32 * (2 * np.arange(len(cy)) - 3), 0, 256 * (hm - 1)))
    # which is the mean of the block's two luma positions where both exist (before rounding and clamping both are exact here)
    tx, _ = HR.luma_tables(h, w, 64, 64, 1.0, (-64.0, -64.0))
    cx2, _ = HR.chroma_tables(h, w, 64, 64, 1.0, (-64.0, -64.0))
    for b in range(w // 2):
        assert 2 * cx2[b] == tx[2 * b] + tx[2 * b + 1]
    if w % 2:  # the odd edge: the centre lies half a pixel right of the last pixel's centre
        assert cx2[-1] == tx[-1] + 16


def test_by_joint_order_is_visible_and_max_is_not():
    scores = np.full((2, 2, 2), 0.9, np.float32)
    a, b = np.zeros((8, 8, 3), np.uint8), np.zeros((8, 8, 3), np.uint8)
    HR.draw_bgr(a, scores, 1.0, mode="joints", joints=(0, 1), alpha=128, alpha_mode="const", palette=PAL)
    HR.draw_bgr(b, scores, 1.0, mode="joints", joints=(1, 0), alpha=128, alpha_mode="const", palette=PAL)
    assert np.array_equal(a, b)  # colours go by place in the list, not by channel: equal maps, equal result
    scores[1] = 0.0
    c = np.zeros((8, 8, 3), np.uint8)
    HR.draw_bgr(c, scores, 1.0, mode="joints", joints=(1, 0), alpha=128, alpha_mode="score", min_score=0.5, palette=PAL)
    want = (PAL[1][1] * ((128 * HR.quantise(0.9) + 2048) >> 12) + 128) >> 8  # only place 1 (channel 0) is blended, in green
    assert (c[:, :, 1] == want).all() and not c[:, :, 0].any() and not c[:, :, 2].any()


# ---- the entries' refusals, without a device -------------------------------------------------------------------------------------------
@pytest.fixture()
def cpu_mode():
    import caffe
    import caffe.pycaffe as pc

    mode = pc._lib.dc_get_mode()
    caffe.set_mode_cpu()
    yield caffe, pc
    pc._lib.dc_set_mode(mode)


def _frames(pc, H, W, fmt, nb, frames=None):
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
    return arr, (y, uv, bgr)


def _style(pc, joints=(0, 1, 2), **fields):
    lut = np.ascontiguousarray(LUT)
    pal = np.ascontiguousarray(PAL, np.uint8)
    j = None if joints is None else np.ascontiguousarray(joints, np.int32)
    st = pc.HeatStyle()
    st.n_joints, st.joints = (0 if j is None else len(j)), (None if j is None else j.ctypes.data)
    st.mode, st.alpha, st.alpha_mode, st.min_score = 0, 128, 1, 0.25
    st.lut, st.palette, st.n_palette = lut.ctypes.data, pal.ctypes.data, 3
    for k, v in fields.items():
        setattr(st, k, v)
    return st, (lut, pal, j)


def _raw(pc, H=20, W=30, fmt=1, nb=2, Cm=3, Hm=5, Wm=6, frames=None, scale=1.0, origin_x=0.0, origin_y=0.0, no_map=False, no_geometry=False,
         no_style=False, **style):
    """dc_draw_heatmap through ctypes with good arguments except what the caller overrides -> (rc, message)."""
    arr, _keep = _frames(pc, H, W, fmt, nb, frames)
    scores = np.zeros((max(nb, 1), max(Cm, 1), max(Hm, 1), max(Wm, 1)), np.float32)
    st, _keep2 = _style(pc, **style)
    g = pc.HeatGeometry(scale, origin_x, origin_y)
    rc = pc._lib.dc_draw_heatmap(arr, nb, H, W, 0, None if no_map else scores.ctypes.data_as(C.c_void_p), 0, Cm, Hm, Wm,
                                 None if no_geometry else C.byref(g), None if no_style else C.byref(st), None)
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
        (dict(frames=frame1("pitch", 29, 0)), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("pitch", 89, 0), fmt=0), ("frame 1", "pitch[0]")),
        (dict(frames=frame1("format", 7)), ("frame 1", "format")),
        (dict(frames=frame1("matrix", 1)), ("frame 1", "matrix", "differs")),
        (dict(frames=frame1("range", 1)), ("frame 1", "range", "differs")),
        (dict(nb=0), ("nb",)), (dict(nb=65), ("nb",)),
        (dict(W=16385), ("width",)), (dict(H=16385, W=1), ("height",)),
        (dict(Cm=0), ("C",)), (dict(Cm=33), ("C",)), (dict(Hm=0), ("Hm",)), (dict(Wm=0), ("Wm",)),
        (dict(scale=nan), ("scale",)), (dict(scale=inf), ("scale",)), (dict(scale=1.0 / 65.0), ("scale",)), (dict(scale=8.001), ("scale",)),
        (dict(scale=0.0), ("scale",)), (dict(scale=-1.0), ("scale",)),
        (dict(origin_x=nan), ("origin_x",)), (dict(origin_x=32768.5), ("origin_x",)), (dict(origin_x=-inf), ("origin_x",)),
        (dict(origin_y=nan), ("origin_y",)), (dict(origin_y=-32769.0), ("origin_y",)),
        (dict(no_geometry=True), ("geometry",)), (dict(no_style=True), ("style",)), (dict(no_map=True), ("map",)),
        (dict(joints=None), ("n_joints",)), (dict(n_joints=33), ("n_joints",)), (dict(joints=None, n_joints=2), ("joints",)),
        (dict(joints=(0, 3)), ("joints[1]", "3")), (dict(joints=(-1, 0)), ("joints[0]", "-1")), (dict(joints=(0, 1, 2), Cm=2), ("joints[2]",)),
        (dict(mode=2), ("mode",)), (dict(mode=-1), ("mode",)),
        (dict(alpha=-1), ("alpha",)), (dict(alpha=257), ("alpha",)),
        (dict(alpha_mode=2), ("alpha_mode",)), (dict(alpha_mode=-1), ("alpha_mode",)),
        (dict(min_score=-0.1), ("min_score",)), (dict(min_score=1.1), ("min_score",)), (dict(min_score=nan), ("min_score",)),
        (dict(lut=None), ("lut",)),
        (dict(mode=1, palette=None), ("palette",)), (dict(mode=1, n_palette=0), ("n_palette",)), (dict(mode=1, n_palette=257), ("n_palette",)),
    ]
    for kw, words in cases:
        rc, msg = _raw(pc, **kw)
        assert rc == EINVAL and "draw_heatmap" in msg and all(w in msg for w in words), (kw, rc, msg)
    # good arguments, both formats, the limits themselves, the table the mode does not use left out: there is no CPU path
    for kw in (dict(), dict(fmt=0), dict(nb=64, Cm=32, joints=tuple(range(32))), dict(joints=(2, 2, 0)), dict(scale=1.0 / 64.0), dict(scale=8.0),
               dict(origin_x=32768.0, origin_y=-32768.0), dict(alpha=0), dict(alpha=256, alpha_mode=0, min_score=1.0),
               dict(mode=1, lut=None), dict(palette=None, n_palette=0)):
        rc, msg = _raw(pc, **kw)
        assert rc == ENOCPU and "CPU mode" in msg, (kw, rc, msg)
    assert pc._lib.dc_draw_heatmap(None, 1, 4, 4, 0, None, 0, 1, 1, 1, None, None, None) == EINVAL
    assert pc._lib.dc_net_draw_heatmap(None, None, 1, 4, 4, 0, None, None) == EINVAL
    assert pc._lib.dc_group_draw_heatmap(None, None, 1, 4, 4, 0, None, 0, 0.0, 0.0, None) == EINVAL


READER = ('name: "r"\ninput: "data"\ninput_dim: %d\ninput_dim: 3\ninput_dim: 16\ninput_dim: 24\n'
          'layer { name: "prob" type: "Convolution" bottom: "data" top: "prob" convolution_param { num_output: 3 kernel_size: 1 stride: 8 bias_term: false } }\n')


def test_net_and_group_entries_check_before_the_cpu_refusal(cpu_mode):
    caffe, pc = cpu_mode
    net = caffe.Net(READER % 2, caffe.TEST, from_text=True)
    img = np.zeros((16, 24, 3), np.uint8)
    two = [caffe.Frame.bgr(img), caffe.Frame.bgr(img.copy())]
    for call in (lambda **kw: net.draw_heatmap(kw.pop("frames", two), **kw), lambda **kw: caffe.NetGroup([net]).draw_heatmap(kw.pop("frames", two), (kw.pop("scale", 1.0),), **kw)):
        for kw, word in ((dict(frames=img), "nb = 1"), (dict(joints=(0, 3)), "joints[1]"), (dict(alpha=300), "alpha"), (dict(scale=9.0), "scale"),
                         (dict(origin=(0.0, float("nan"))), "origin_y"), (dict(min_score=2.0), "min_score")):
            with pytest.raises(caffe.DeepcutError) as ei:
                call(**kw)
            assert ei.value.code == EINVAL and "draw_heatmap" in str(ei.value) and word in str(ei.value), (kw, str(ei.value))
        with pytest.raises(caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == ENOCPU
    grp = caffe.NetGroup([net])
    with pytest.raises(ValueError, match="one scale per group member"):
        grp.draw_heatmap(two, (1.0, 0.5))
    with pytest.raises(caffe.DeepcutError) as ei:
        grp.draw_heatmap(two, (1.0,), base=1)
    assert ei.value.code == EINVAL and "base" in str(ei.value)
    assert not img.any()


def test_python_entry_refusals_and_tables(cpu_mode):
    caffe, _pc = cpu_mode
    import pose

    img = np.zeros((20, 30, 3), np.uint8)
    scores = np.ones((3, 5, 6), np.float32)
    frozen = img.copy()
    frozen.flags.writeable = False
    with pytest.raises(ValueError, match="writable"):
        caffe.draw_heatmap(frozen, scores, 1.0)
    with pytest.raises(ValueError, match="frames"):
        caffe.draw_heatmap("picture", scores, 1.0)
    with pytest.raises(ValueError, match="mode"):
        caffe.draw_heatmap(img, scores, 1.0, mode="rainbow")
    with pytest.raises(ValueError, match="alpha_mode"):
        caffe.draw_heatmap(img, scores, 1.0, alpha_mode="linear")
    with pytest.raises(ValueError, match="one map per frame"):
        caffe.draw_heatmap(img, np.ones((2, 3, 5, 6), np.float32), 1.0)
    with pytest.raises(ValueError, match="lut"):
        caffe.draw_heatmap(img, scores, 1.0, lut=np.zeros((16, 3), np.uint8))
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.draw_heatmap(img, scores, 1.0, joints=(0, 5))
    assert ei.value.code == EINVAL and "joints[1]" in str(ei.value)
    for call in (lambda: caffe.draw_heatmap(img, scores, 0.5, origin=(3.5, -2.0), mode="joints", joints=(2, 0, 2)),
                 lambda: caffe.draw_heatmap([caffe.Frame.bgr(img), caffe.Frame.bgr(img.copy())], np.ones((2, 3, 5, 6)), 1.0, alpha_mode="const"),
                 lambda: pose.draw_heatmap(img, scores, 1.0)):
        with pytest.raises(caffe.DeepcutError) as ei:
            call()
        assert ei.value.code == ENOCPU
    assert not img.any()
    lut = np.asarray(caffe.HEAT_LUT)
    assert lut.shape == (256, 3) and lut.min() >= 0 and lut.max() <= 255 and tuple(lut[0]) == (0, 0, 0) and tuple(lut[255]) == (255, 255, 255)
    assert len(set(map(tuple, lut))) == 256  # a ramp: no two scores share a colour

"""GPU: `caffe.draw_heatmap` / `Net.draw_heatmap` / `NetGroup.draw_heatmap` (dc_draw_heatmap and its net and group forms) against the
numpy restatement of the rule in tests/heat_ref.py, BYTE FOR BYTE, the pitch padding (pre-filled with a sentinel) included — the rule is
integer from the first quantisation on and the quantisation is correctly rounded float32 on both sides, so there is no tolerance.

PARITY UNPINNED BY THE REFERENCE: its demo draws 14 numpy circles and never shows a map; the rule is this project's own.

Shapes: a 37 x 45 frame (odd both ways: 2 x 2 tiles of 32 x 32 with partial edge tiles, chroma blocks of 2 and 1 pixels) over a 5 x 6-cell
map of 3 channels; a 64 x 64 frame at scale 8 over 32 channels for the largest patch a workgroup stages (34 x 34 cells x 32 channels)."""
import numpy as np
import pytest

import heat_ref as HR
import sparse_head_ref as SR
from test_gpu_draw import SENT, Bgr, Nv12

pytestmark = pytest.mark.gpu

H, W = 37, 45
LUT = np.stack([np.arange(256), 255 - np.arange(256), (np.arange(256) * 7) % 256], axis=1).astype(np.uint8)
PAL = ((255, 0, 0), (0, 255, 0), (30, 60, 255), (0, 245, 255), (255, 131, 250))
FORMATS = {"bgr": None, "nv12-601-limited": ("bt601", "limited"), "nv12-709-full": ("bt709", "full")}
# scale, origin: cell centres on pixel centres; two frame pixels per network pixel; ties (256 u = x / 2 + 1/2 ... exact halves at odd x);
# a fractional scale and origin; the largest scale; the whole map off-frame to the left, so every column clamps
GEOMETRIES = {"one": (1.0, (0.0, 0.0)), "half": (0.5, (0.0, 0.0)), "ties": (1.0 / 64.0, (-255.5, -254.5)), "odd": (1.37, (2.25, -3.5)),
              "eight": (8.0, (0.0, 0.0)), "off-frame": (1.0, (-1000.0, 1.5))}


def _surface(fmt, h=H, w=W, seed=3):
    if fmt == "bgr":
        return Bgr(h, w, 3 * w + 13, seed)
    return Nv12(h, w, w + 7, 2 * ((w + 1) // 2) + 10, seed, *FORMATS[fmt])


def _scores(seed=5, nb=1, c=3, hm=5, wm=6):
    """Values on both sides of [0, 1], with NaN, -0.0, a negative and a value above 1 planted in every image."""
    rs = np.random.RandomState(seed)
    s = rs.uniform(-0.2, 1.2, (nb, c, hm, wm)).astype(np.float32)
    s[:, 0, 0, 0], s[:, -1, 1, 2], s[:, 0, 2, 1], s[:, -1, hm - 1, wm - 1] = np.nan, -0.0, -7.0, 3.5
    return s


def _reference(surfaces, scores, scale, origin, style):
    want = [s.copy() for s in surfaces]
    for b, s in enumerate(want):
        if isinstance(s, Nv12):
            y, uv = s.views()
            HR.draw_nv12(y, uv, scores[b], scale, origin, s.matrix, s.range, **style)
        else:
            HR.draw_bgr(s.views()[0], scores[b], scale, origin, **style)
    return want


def _on_host(caffe, surfaces, draw):
    got = [s.copy() for s in surfaces]
    draw([s.host_frame(caffe) for s in got])
    return got


def _on_device(caffe, surfaces, draw):
    import torch

    tensors = [[torch.from_numpy(b).cuda() for b in s.bufs] for s in surfaces]
    torch.cuda.synchronize()
    draw([s.device_frame(caffe, t) for s, t in zip(surfaces, tensors)])
    got = [s.copy() for s in surfaces]
    for g, t in zip(got, tensors):
        g.bufs = [x.cpu().numpy() for x in t]
    return got


def _equal(got, want, what):
    for b, (g, w_) in enumerate(zip(got, want)):
        for k, (x, y) in enumerate(zip(g.bufs, w_.bufs)):
            bad = np.argwhere(x != y)
            assert bad.size == 0, "%s frame %d plane %d: %d bytes differ, first at %s: got %d, want %d" % (
                what, b, k, len(bad), tuple(bad[0]), x[tuple(bad[0])], y[tuple(bad[0])])


def _same(a, b):
    return all(np.array_equal(x, y) for s, t in zip(a, b) for x, y in zip(s.bufs, t.bufs))


def _check(caffe, surfaces, scores, scale, origin=(0.0, 0.0), where=("host", "device"), draw=None, **style):
    """Host and device frames against the restatement (padding included); -> the restatement's surfaces.  draw(frames): the call under
    test, by default `caffe.draw_heatmap` on the scores."""
    want = _reference(surfaces, scores, scale, origin, style)
    if draw is None:
        draw = lambda frames: caffe.draw_heatmap(frames, scores, scale, origin=origin, **style)  # noqa: E731
    for place in where:
        _equal((_on_host if place == "host" else _on_device)(caffe, surfaces, draw), want, "%s %r" % (place, style))
    return want


MAX = dict(mode="max", alpha=200, alpha_mode="score", min_score=0.2, lut=LUT)
JOINTS = dict(mode="joints", alpha=160, alpha_mode="const", min_score=0.35, palette=PAL, joints=(2, 0, 2, 1))  # a repeat and a reordering


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
def test_formats_and_geometries_match_the_restatement(gpu_caffe, fmt, geometry):
    scale, origin = GEOMETRIES[geometry]
    s = _surface(fmt)
    scores = _scores()
    for style in (MAX, JOINTS):
        want = _check(gpu_caffe, [s], scores, scale, origin, **style)
        assert not _same(want, [s])  # something was blended
        for buf in want[0].bufs:  # and the restatement itself left the padding alone
            assert (buf[:, -7:] == SENT).all()
    if geometry == "ties":
        tx, _ = HR.luma_tables(H, W, 5, 6, scale, origin)
        assert tx[:8].tolist() == [0, 0, 1, 2, 2, 2, 3, 4]
    if geometry == "off-frame":
        tx, _ = HR.luma_tables(H, W, 5, 6, scale, origin)
        assert (tx == 256 * 5).all()


@pytest.mark.parametrize("fmt", ["bgr", "nv12-601-limited"])
def test_modes_alpha_modes_and_alpha_limits(gpu_caffe, fmt):
    s = _surface(fmt, seed=8)
    scores = _scores(6)
    for mode in ("max", "joints"):
        for alpha_mode in ("const", "score"):
            for alpha in (0, 1, 255, 256):
                style = dict(mode=mode, alpha=alpha, alpha_mode=alpha_mode, min_score=0.0, lut=LUT, palette=PAL)
                want = _check(gpu_caffe, [s], scores, 1.37, (2.25, -3.5), **style)
                # alpha 0 blends nothing; alpha 1 scaled by a score <= 1 rounds to 0 except at a full score
                assert _same(want, [s]) == (alpha == 0), (mode, alpha_mode, alpha)
    # joint lists: order is visible in "joints" mode, a repeat is drawn twice
    a = _check(gpu_caffe, [s], scores, 1.0, **dict(JOINTS, joints=(0, 1, 2)))
    b = _check(gpu_caffe, [s], scores, 1.0, **dict(JOINTS, joints=(2, 1, 0)))
    c = _check(gpu_caffe, [s], scores, 1.0, **dict(JOINTS, joints=(0, 1, 2, 0)))
    assert not _same(a, b) and not _same(a, c)
    d = _check(gpu_caffe, [s], scores, 1.0, **dict(MAX, joints=(1,)))
    assert not _same(d, _check(gpu_caffe, [s], scores, 1.0, where=(), **MAX))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_tile_below_min_score_is_left_untouched(gpu_caffe, fmt):
    """At scale 1 tile (1, 1) — pixels 32.. of both axes — reaches map rows 3..4 and columns 3..5 only: with those below min_score the
    workgroup returns before loading a pixel; the other three tiles are blended as ever."""
    scores = np.full((1, 3, 5, 6), 0.9, np.float32)
    scores[0, :, 3:, 3:] = 0.1
    scores[0, 1, 0, 0] = np.nan
    s = _surface(fmt, seed=12)
    for style in (dict(MAX, min_score=0.5), dict(JOINTS, min_score=0.5), dict(MAX, min_score=0.0, alpha=3)):  # the last: A(v) = 0 below the gate
        want = _check(gpu_caffe, [s], scores, 1.0, **style)
        for v, u in zip(want[0].views(), s.views()):
            if v.shape[:2] == (H, W):
                assert np.array_equal(v[32:, 32:], u[32:, 32:]) and not np.array_equal(v[:32, :32], u[:32, :32])
            else:
                assert np.array_equal(v[16:, 16:], u[16:, 16:]) and not np.array_equal(v[:16, :16], u[:16, :16])


@pytest.mark.parametrize("fmt", ["bgr", "nv12-709-full"])
def test_thirty_two_channels_at_scale_eight_the_largest_patch(gpu_caffe, fmt):
    """64 x 64 pixels at scale 8 reach 64 x 64 cells: every tile stages 33 or 34 cells per side of all 32 channels (74 KB of LDS), and
    the staging loop runs more than a hundred trips per thread."""
    rs = np.random.RandomState(17)
    scores = rs.uniform(-0.1, 1.1, (1, 32, 64, 64)).astype(np.float32)
    s = _surface(fmt, 64, 64, seed=13)
    _check(gpu_caffe, [s], scores, 8.0, (0.0, 0.0), **dict(MAX, joints=None))
    _check(gpu_caffe, [s], scores, 8.0, (0.25, -0.5), **dict(JOINTS, joints=tuple(range(32))))


@pytest.mark.parametrize("fmt", ["bgr", "nv12-601-limited"])
def test_three_frames_one_call_and_repeats(gpu_caffe, fmt):
    surfaces = [_surface(fmt, seed=20 + b) for b in range(3)]
    scores = _scores(9, nb=3)
    want = _check(gpu_caffe, surfaces, scores, 0.5, (1.0, 2.0), **MAX)
    again = _on_device(gpu_caffe, surfaces, lambda frames: gpu_caffe.draw_heatmap(frames, scores, 0.5, origin=(1.0, 2.0), **MAX))
    assert _same(again, want)
    if fmt == "bgr":  # a bare array is wrapped like Frame.bgr and drawn in place; a caller's stream is taken
        import torch

        img = np.ascontiguousarray(surfaces[0].views()[0])
        gpu_caffe.draw_heatmap(img, scores[0], 0.5, origin=(1.0, 2.0), **MAX)
        assert np.array_equal(img, want[0].views()[0])
        t = [torch.from_numpy(b).cuda() for b in surfaces[1].bufs]
        st = torch.cuda.Stream()
        torch.cuda.synchronize()
        gpu_caffe.draw_heatmap(surfaces[1].device_frame(gpu_caffe, t), scores[1], 0.5, origin=(1.0, 2.0), stream=st.cuda_stream, **MAX)
        assert np.array_equal(t[0].cpu().numpy(), want[1].bufs[0])


def test_a_device_map_is_read_where_it_is(gpu_caffe):
    """dc_draw_heatmap with map_is_device = 1, through ctypes: the same bytes as with the host map."""
    import ctypes as C

    import torch

    import caffe.pycaffe as pc

    s = _surface("nv12-601-limited", seed=31)
    scores = _scores(10)
    want = _reference([s], scores, 1.37, (0.0, 0.0), MAX)
    got = s.copy()
    frame = got.host_frame(gpu_caffe)
    arr, h, w, is_device = pc._frame_array([frame])
    st, _keep = pc._heat_style(3, None, MAX["mode"], MAX["alpha"], MAX["alpha_mode"], MAX["min_score"], LUT, None)
    g = pc.HeatGeometry(1.37, 0.0, 0.0)
    dev = torch.from_numpy(scores).cuda()
    torch.cuda.synchronize()
    assert pc._lib.dc_draw_heatmap(arr, 1, h, w, 0, C.c_void_p(dev.data_ptr()), 1, 3, 5, 6, C.byref(g), C.byref(st), None) == 0
    _equal([got], want, "device map")


# ---- the net's own maps, in its element type --------------------------------------------------------------------------------------------
J = 14


def reader_prototxt(n, h, w):
    """The reader net of tests/test_gpu_map_readers.py: an input feeding three 1 x 1 stride-8 convolutions named like the maps."""
    L = ['name: "map_reader"', 'input: "data"'] + ["input_dim: %d" % d for d in (n, 3, h * 8, w * 8)]
    for top, c in (("prob", J), ("loc_pred", 2 * J), ("next_pred", 364)):
        L.append('layer { name: "%s" type: "Convolution" bottom: "data" top: "%s" convolution_param { num_output: %d kernel_size: 1 '
                 "stride: 8 bias_term: false } }" % (top, top, c))
    return "\n".join(L) + "\n"


def _plant(net, prob):
    """The net forwarded once at the map's size, then its `prob` overwritten through .data; -> the values read back (the net's element
    type widened to float32: what the device will read)."""
    n, _, h, w = prob.shape
    net.blobs["data"].reshape(n, 3, h * 8, w * 8)
    net.reshape()
    net.blobs["data"].data[...] = 0
    net.forward()
    net.blobs["prob"].data[...] = prob
    return np.array(net.blobs["prob"].data, np.float32)


@pytest.fixture(scope="module", params=["f32", "f16", "bf16"])
def reader(request, gpu_caffe):
    net = gpu_caffe.Net(reader_prototxt(1, 2, 2), gpu_caffe.TEST, from_text=True, fuse=0, dtype=request.param)
    for blobs in net.params.values():
        blobs[0].data[...] = 0
    assert net.dtype == request.param
    return net


@pytest.mark.parametrize("fmt", ["bgr", "nv12-601-limited"])
def test_net_entry_reads_the_nets_element_type(gpu_caffe, reader, fmt):
    """Crafted maps planted through .data and read back: the restatement, the stand-alone call on the read-back values and the net's
    entry give the same bytes; a one-member group's entry equals the member's."""
    crafted = _scores(11, nb=2, c=J)
    crafted[:, 3] = np.linspace(0.0, 1.0, 30, dtype=np.float32).reshape(5, 6) + np.float32(1.0 / 8192.0)  # values 16-bit types must round
    # what comes back through .data is the host's float32 copy; the upload the map reader triggers rounds it to the net's element type
    # (nearest, ties to even): the restatement gets the values the device reads
    back = SR.round_to(_plant(reader, crafted), reader.dtype)
    if reader.dtype != "f32":
        assert not np.array_equal(back[:, 3], crafted[:, 3])
    surfaces = [_surface(fmt, seed=40), _surface(fmt, seed=41)]
    grp = gpu_caffe.NetGroup([reader])
    for style in (dict(MAX, joints=(3, 0, 13)), dict(JOINTS, joints=(13, 3, 3, 0))):
        want = _check(gpu_caffe, surfaces, back, 1.37, (2.25, -3.5), **style)
        net_style = {k: v for k, v in style.items()}
        _check(gpu_caffe, surfaces, back, 1.37, (2.25, -3.5), draw=lambda frames: reader.draw_heatmap(frames, 1.37, origin=(2.25, -3.5), **net_style),
               **style)
        got = _on_device(gpu_caffe, surfaces, lambda frames: grp.draw_heatmap(frames, (1.37,), origin=(2.25, -3.5), **net_style))
        _equal(got, want, "one-member group")
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        reader.draw_heatmap(surfaces[0].host_frame(gpu_caffe), 1.0)
    assert ei.value.code == -1 and "nb = 1" in str(ei.value)


def test_before_a_forward_the_map_readers_own_refusal_is_passed_on(gpu_caffe):
    net = gpu_caffe.Net(reader_prototxt(1, 2, 2), gpu_caffe.TEST, from_text=True, fuse=0)
    s = _surface("bgr", 16, 16)
    with pytest.raises(gpu_caffe.DeepcutError) as ei:
        net.draw_heatmap(s.host_frame(gpu_caffe), 1.0, lut=LUT)
    assert ei.value.code == -1 and "forward" in str(ei.value)
    assert (s.bufs[0][:, -13:] == SENT).all()


def heads_prototxt(n, h5, w5, h, w):
    """The three sibling heads of tests/test_gpu_tile_shapes.py (net 4) at a small size: at DC_OPT_FUSE 2 ONE 86-channel deconvolution
    with the cropped window, the skip sum and the sigmoid prefix, whose tops are channel views of the merged tensor."""
    t = ('input: "low" input_dim: %d input_dim: 256 input_dim: %d input_dim: %d\n' % (n, h5, w5) +
         'input: "hi" input_dim: %d input_dim: 128 input_dim: %d input_dim: %d\n' % (n, h, w))
    conv = ('layer { name: "%s" type: "%s" bottom: "%s" top: "%s" convolution_param { num_output: %d kernel_size: %d pad: 0 stride: %d dilation: 1 '
            "bias_term: true } }\n")
    for k, c in enumerate((J, 2 * J, 44)):
        t += conv % ("up%d" % k, "Deconvolution", "low", "up%d" % k, c, 3, 2) + conv % ("skip%d" % k, "Convolution", "hi", "skip%d" % k, c, 1, 1)
        t += 'layer { name: "crop%d" type: "Crop" bottom: "up%d" bottom: "skip%d" top: "up%dc" }\n' % (k, k, k, k)
        t += 'layer { name: "sum%d" type: "Eltwise" bottom: "skip%d" bottom: "up%dc" top: "sum%d" }\n' % (k, k, k, k)
    return t + 'layer { name: "prob" type: "Sigmoid" bottom: "sum0" top: "prob" }\n'


def test_merged_heads_one_real_forward(gpu_caffe):
    """A head-only net at DC_OPT_FUSE 2: `prob` is a channel view of the merged head tensor (cp = 86, not C = 14).  The entry on the view
    equals the stand-alone call on the map the net hands out."""
    net = gpu_caffe.Net(heads_prototxt(2, 3, 4, 5, 6), gpu_caffe.TEST, from_text=True, fuse=2)
    rs = np.random.RandomState(23)
    for blobs in net.params.values():
        for p in blobs:
            p.data[...] = rs.uniform(-0.08, 0.08, p.data.shape)
    for name in ("low", "hi"):
        net.blobs[name].data[...] = rs.uniform(-1, 1, net.blobs[name].data.shape)
    net.forward()
    assert "up0+crop0+sum0+prob" in net.plan_text(), net.plan_text()  # the heads were merged
    surfaces = [_surface("nv12-709-full", seed=50), _surface("nv12-709-full", seed=51)]
    style = dict(JOINTS, joints=(13, 0, 7, 7), min_score=0.5)
    got = _on_device(gpu_caffe, surfaces, lambda frames: net.draw_heatmap(frames, 1.0, **style))
    prob = np.array(net.blobs["prob"].data, np.float32)
    assert prob.shape == (2, J, 5, 6) and prob.min() > 0.0 and prob.max() < 1.0 and prob.std() > 0.01
    _equal(got, _check(gpu_caffe, surfaces, prob, 1.0, **style), "merged heads")


def test_two_scale_group_draws_its_fused_map_and_disturbs_nothing(gpu_caffe):
    """A group of a reader net and its clone at another map size: the group's entry equals the stand-alone call on
    fuse_maps(want=("prob",)); the people path's results on the shared fused buffer, and draw_people's on the shared overlay buffer, are
    what they were before the heat-map calls."""
    a = gpu_caffe.Net(reader_prototxt(1, 2, 2), gpu_caffe.TEST, from_text=True, fuse=0)
    for blobs in a.params.values():
        blobs[0].data[...] = 0
    b = a.clone()
    rs = np.random.RandomState(29)
    scales = (1.0, 0.75)
    for net, (hm, wm) in ((a, (5, 6)), (b, (4, 5))):
        _plant(net, rs.uniform(0.0, 1.0, (1, J, hm, wm)).astype(np.float32))
        net.blobs["loc_pred"].data[...] = rs.uniform(-0.5, 0.5, net.blobs["loc_pred"].data.shape)
    grp = gpu_caffe.NetGroup([a, b])
    parts_before = grp.detect_parts(scales, 0, 0.2, 1, 8)
    people = np.array([[[10.0, 12.0, 1.0]] * J, [[30.0, 20.0, 1.0]] * J])
    s = _surface("nv12-601-limited", seed=60)
    drawn_before = _on_device(gpu_caffe, [s], lambda frames: gpu_caffe.draw_people(frames, people, joint_radius=5.0))
    for base in (0, 1):
        fused = grp.fuse_maps(scales, base, want=("prob",))["prob"]
        assert fused.shape == ((1, J, 5, 6), (1, J, 4, 5))[base]
        want = _check(gpu_caffe, [s], fused, scales[base], (0.5, 0.25), **MAX)
        for where in (_on_host, _on_device):
            _equal(where(gpu_caffe, [s], lambda frames: grp.draw_heatmap(frames, scales, base=base, origin=(0.5, 0.25), **MAX)), want, "group")
    # the clone taken as the mirrored member: the same plan check_mirror hands to fuse_maps, so the fused map is already un-mirrored
    mkw = dict(mirror=(0, 1), image_width=W, joint_mirror=(5, 4, 3, 2, 1, 0, 11, 10, 9, 8, 7, 6, 12, 13))
    flipped = grp.fuse_maps(scales, 0, want=("prob",), **mkw)["prob"]
    assert not np.array_equal(flipped, grp.fuse_maps(scales, 0, want=("prob",))["prob"])
    want = _check(gpu_caffe, [s], flipped, scales[0], **JOINTS)
    _equal(_on_device(gpu_caffe, [s], lambda frames: grp.draw_heatmap(frames, scales, **dict(JOINTS, **mkw))), want, "mirrored group")
    parts_after = grp.detect_parts(scales, 0, 0.2, 1, 8)
    assert np.array_equal(parts_before[0], parts_after[0]) and np.array_equal(parts_before[1], parts_after[1])
    assert _same(_on_device(gpu_caffe, [s], lambda frames: gpu_caffe.draw_people(frames, people, joint_radius=5.0)), drawn_before)


# ---- pose_demo.py --heatmap ---------------------------------------------------------------------------------------------------------------
def test_demo_heatmap_writes_its_png_beside_the_unchanged_outputs(synth152, tmp_path):
    """The demo's command line with --heatmap: `<out>_heat.png` is the image with something blended into it, and the pose and the
    `_vis.png` are what the demo writes without the flag — the numpy discs of the pose it saved."""
    import os
    import subprocess
    import sys

    from PIL import Image

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    demo = os.path.join(root, "deepcut-cnn_amd", "python", "pose", "pose_demo.py")
    rgb = np.random.RandomState(8).randint(0, 256, (96, 128, 3)).astype(np.uint8)
    Image.fromarray(rgb).save(str(tmp_path / "img.png"))
    out = str(tmp_path / "pose.npz")
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.join(root, "deepcut-cnn_amd", "python"), root]))
    r = subprocess.run([sys.executable, demo, str(tmp_path / "img.png"), "--model_bin", synth152[0], "--out_name", out, "--heatmap", "joints"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    pose = np.load(out, allow_pickle=True)["pose"]
    heat = np.asarray(Image.open(out + "_heat.png"))
    assert heat.shape == rgb.shape and not np.array_equal(heat, rgb)
    from pose import pose_demo as PD

    vis = rgb.copy()
    for j in range(14):
        PD.draw_disc(vis, pose[0, j], pose[1, j], 8, PD.COLORS[j])
    assert np.array_equal(np.asarray(Image.open(out + "_vis.png")), vis)

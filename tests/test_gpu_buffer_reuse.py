"""-m gpu: the grow-only device buffers behind the host entries (csrc/net.h DevBuf: uploaded images, staged frame planes and their plane
table, the horizontally resampled rows, the box table, the pose staging, the readers' scratch, the kept assembly table, the group's
scratch) when a buffer that has grown serves a smaller call and then a larger one again.

NO TOLERANCE: every assertion is bit-for-bit equality between a net that went through the whole size sequence and a fresh net that only
ever saw that one size.  What the fresh net answers is pinned elsewhere, against the float64 and Pillow restatements:
tests/test_gpu_map_readers.py, test_gpu_preprocess.py, test_gpu_frames.py, test_gpu_boxes.py, test_gpu_people.py.

THE NET is the three-convolution reader net of tests/test_gpu_map_readers.py (1 x 1, stride 8, DC_OPT_FUSE 0), float32.  The reader cases
plant their maps through `.data`, as that file does.  The image, frame and box cases run it with random filters, so that the maps are a
function of the pixels the pre-processing delivers; sequence net and fresh nets are clones of one net there: the same filters in HBM and
the same tile per layer signature (the tune cache is the model's), every buffer named above each clone's own."""
import numpy as np
import pytest

import map_reader_cases as MC
from test_gpu_map_readers import MAPS, Reader, reader_prototxt

pytestmark = pytest.mark.gpu

MAP_STEPS = ((1, 2, 2), (3, 6, 5), (1, 2, 2), (3, 6, 5))  # (batch, map rows, map columns): grown, smaller, larger again
IMAGE_STEPS = ((1, 24, 20), (2, 56, 72), (1, 24, 20))     # (images, height, width)
SCALES = (1.0, 0.75)                                      # 0.75: both resample passes, the horizontal one through its row buffer
EDGES = [(a, c) for a in range(MC.J) for c in range(MC.J) if a != c]  # 182 = 364 / 2 regression edges


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), what


def _same_dict(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        _same(got[k], want[k], what + (k,))


def _maps(n, h, w, seed):
    """prob over the whole of [0, 1), loc_pred and next_pred multiples of 1/8: different for every size, image, joint and cell."""
    prob = np.stack([np.stack([MC.background(h, w, j + 3 * b + seed, below=256) for j in range(MC.J)]) for b in range(n)])
    nxt = (np.random.RandomState(seed).randint(-16, 17, (n, 364, h, w)) / 8.0).astype(np.float32)
    return prob, MC.loc_map(n, h, w, seed), nxt


def _plant(rd, prob, loc, nxt):
    rd.plant(prob, loc)
    rd.net.blobs["next_pred"].data[...] = nxt


def _readers(rd):
    counts, dets = rd.net.detect_parts(1.0, 0.25, 1, 6)
    gcounts, gdets = rd.grp.detect_parts((1.0,), 0, 0.25, 1, 6)
    return {"counts": counts, "dets": dets, "pose": rd.net.decode_pose(0.75), "group counts": gcounts, "group dets": gdets,
            "group pose": rd.grp.decode_pose((0.75,), 0)}


def test_map_readers_after_growth_and_a_smaller_call(gpu_caffe):
    seq = Reader(gpu_caffe, "f32")
    for step, (n, h, w) in enumerate(MAP_STEPS):
        maps = _maps(n, h, w, step % 2)
        _plant(seq, *maps)
        fresh = Reader(gpu_caffe, "f32")
        _plant(fresh, *maps)
        _same_dict(_readers(seq), _readers(fresh), ("readers", step))


def _people(rd, edges):
    kw = dict(threshold=0.25, radius=1, max_det=6, edges=edges, max_cost=1e6, seed_threshold=0.3, max_people=8)
    out = {}
    for who, people in (("net", rd.net.assemble_people(1.0, **kw)), ("group", rd.grp.assemble_people((1.0,), 0, **kw))):
        out[who + " n_people"] = np.array([len(p["people"]) for p in people])
        for b, p in enumerate(people):
            out["%s people %d" % (who, b)], out["%s cand %d" % (who, b)] = p["people"], p["cand"]
    return out


def test_people_after_growth_and_another_edge_list(gpu_caffe):
    """The sizes of the reader case, and between them a call with another edge list of the same length: the table kept on the device is
    uploaded again into the buffer it has."""
    other = EDGES[::-1]
    seq = Reader(gpu_caffe, "f32")
    found = 0
    for step, ((n, h, w), edges) in enumerate(((MAP_STEPS[0], EDGES), (MAP_STEPS[1], EDGES), (MAP_STEPS[1], other), (MAP_STEPS[2], EDGES),
                                               (MAP_STEPS[3], EDGES))):
        maps = _maps(n, h, w, step % 2)
        _plant(seq, *maps)
        fresh = Reader(gpu_caffe, "f32")
        _plant(fresh, *maps)
        want = _people(fresh, edges)
        _same_dict(_people(seq, edges), want, ("people", step))
        found += int(want["net n_people"].sum())
    assert found > 0  # (the equalities are not those of empty lists)


@pytest.fixture(scope="module")
def model(gpu_caffe):
    """The reader net with random filters: what its clones share."""
    net = gpu_caffe.Net(reader_prototxt(1, 3, 3), gpu_caffe.TEST, from_text=True, fuse=0, dtype="f32")
    rs = np.random.RandomState(3)
    for blobs in net.params.values():
        blobs[0].data[...] = rs.randn(*blobs[0].data.shape) / 64
    return net


def _images(n, h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)


def test_host_images_after_growth_and_a_smaller_call(model):
    seq = model.clone()
    for step, (n, h, w) in enumerate(IMAGE_STEPS):
        x = _images(n, h, w, step)
        for scale in SCALES:
            got = seq.forward_images(x, scale, want=MAPS, pose=True)
            want = model.clone().forward_images(x, scale, want=MAPS, pose=True)
            assert np.abs(want["loc_pred"]).max() > 0
            _same_dict(got, want, ("images", step, scale))


def _nv12_frames(caffe, n, h, w, seed):
    """n host NV12 frames whose rows are views into wider buffers (pitch = width + 11 / chroma row + 6), padding 0xFF."""
    rs = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    frames = []
    for _ in range(n):
        ybuf, uvbuf = np.full((h, w + 11), 0xFF, np.uint8), np.full((ch, 2 * cw + 6), 0xFF, np.uint8)
        y, uv = ybuf[:, :w], np.lib.stride_tricks.as_strided(uvbuf, (ch, cw, 2), (2 * cw + 6, 2, 1))
        y[...] = rs.randint(0, 256, (h, w))
        uv[...] = rs.randint(0, 256, (ch, cw, 2))
        frames.append(caffe.Frame.nv12(y, uv))
        assert frames[-1].pitches == [w + 11, 2 * cw + 6]
    return frames


def test_host_nv12_frames_after_growth_and_a_smaller_call(gpu_caffe, model):
    seq = model.clone()
    for step, (n, h, w) in enumerate(IMAGE_STEPS):
        frames = _nv12_frames(gpu_caffe, n, h, w, step)
        for scale in SCALES:
            got = seq.forward_images(frames, scale, want=MAPS, pose=True)
            want = model.clone().forward_images(frames, scale, want=MAPS, pose=True)
            assert np.abs(want["loc_pred"]).max() > 0
            _same_dict(got, want, ("frames", step, scale))


BOX_IMAGE_HW, BOX_CANVAS = (64, 80), (32, 40)
BOX_STEPS = (([(5, 3, 41, 33)], [1.0]),
             ([(0, 0, 40, 32), (20, 10, 55, 40), (44, 34, 80, 64)], [1.0, 0.75, 1.0]),
             ([(5, 3, 41, 33)], [1.0]))


def _boxes(net, grp, img, boxes, scales):
    """Net.forward_boxes with its decode, then the same boxes through the one-member group of that net and its decode_boxes."""
    out = net.forward_boxes(img, boxes, scales, canvas=BOX_CANVAS, want=MAPS, pose=True)
    grp.forward_boxes(img, boxes, (1.0,), scales, canvas=BOX_CANVAS, want=(), pose=False)
    for k, v in grp.decode_boxes((1.0,), 0, want=MAPS).items():
        out["group " + k] = v
    return out


def test_boxes_after_growth_and_a_smaller_call(gpu_caffe, model):
    img = _images(1, BOX_IMAGE_HW[0], BOX_IMAGE_HW[1], 9)[0]
    seq = model.clone()
    seq_grp = gpu_caffe.NetGroup([seq])
    for step, (boxes, scales) in enumerate(BOX_STEPS):
        got = _boxes(seq, seq_grp, img, boxes, scales)
        fresh = model.clone()
        want = _boxes(fresh, gpu_caffe.NetGroup([fresh]), img, boxes, scales)
        assert want["pose"].shape == (len(boxes), 5, MC.J) and np.abs(want["loc_pred"]).max() > 0
        _same_dict(got, want, ("boxes", step))

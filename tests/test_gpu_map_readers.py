"""-m gpu: the device map readers of csrc/pose.hip on the crafted maps of tests/map_reader_cases.py — exact ties, map edges, the sort
boundaries of part_select_kernel, both signs of zero, NaN cells, boxes whose own cells exclude the global maximum — against
`pose_from_maps`, `oracle.multiperson.nms_candidates` and `boxfuse_ref.box_poses`, on float32, float16 and bfloat16 nets.

READER NET: the readers look `prob`, `loc_pred` and `next_pred` up by name, so an input feeding three 1 x 1 stride-8 Convolutions with
those tops (14, 28 and 364 channels, DC_OPT_FUSE 0) is a net of any map size whose blobs are written through `.data` after one forward
(host-authoritative: Net::map_ref and Net::decode_pose upload them in the net's own element type).  Every entry below accepted it:
Net.decode_pose, Net.detect_parts, and NetGroup.decode_pose / detect_parts / decode_boxes on a group of that one member (the group's
forward_boxes included), whose fused maps are the member's own widened to float32.

MERGED LAYOUT (DC_OPT_FUSE 2, the maps as channel views with pcp != C and pc0 != 0): tried once on the 152-layer net, whose heads are
the only ones the lowering merges; a write through `.data` of a view does NOT reach the readers (they read the merged head tensor on the
device, which nothing uploads to), so the crafted maps cannot be planted there.  That layout stays with the real forwards of
tests/test_gpu_fullnet.py::test_device_pose_decode_equals_host_decode and tests/test_gpu_multiperson.py.

EXACT: counts, scores, rows, cols, the candidate order and pose[2] are compared with array_equal, positions with rtol=0, atol=1e-9 (the
device evaluates cell * 8 + 4 + loc * sqrt(53) in its own order) as tests/test_gpu_multiperson.py does.  A tie goes to the cell the rule
names or the test fails.

PARITY: `pose_from_maps` is pinned to the reference's `_pose_from_mats` (tests/test_pose.py); the candidates, the fusion and the box
entry have no reference counterpart (the reference stops at the maps): the rules are include/deepcut_hip.h's."""
import numpy as np
import pytest

import map_reader_cases as MC
from pose import estimate_pose as ep

pytestmark = pytest.mark.gpu

MAPS = ("prob", "loc_pred")
STRIDE = 8


def reader_prototxt(n, h, w):
    L = ['name: "map_reader"', 'input: "data"'] + ["input_dim: %d" % d for d in (n, 3, h * STRIDE, w * STRIDE)]
    for top, c in (("prob", MC.J), ("loc_pred", 2 * MC.J), ("next_pred", 364)):
        L.append('layer { name: "%s" type: "Convolution" bottom: "data" top: "%s" convolution_param { num_output: %d kernel_size: 1 '
                 "stride: %d bias_term: false } }" % (top, top, c, STRIDE))
    return "\n".join(L) + "\n"


class Reader(object):
    """One reader net of one element type and the group of that one member."""

    def __init__(self, caffe, kind):
        self.kind = kind
        self.net = caffe.Net(reader_prototxt(1, 2, 2), caffe.TEST, from_text=True, fuse=0, dtype=kind)
        for blobs in self.net.params.values():
            blobs[0].data[...] = 0
        self.grp = caffe.NetGroup([self.net])
        assert self.net.dtype == kind

    def write(self, prob, loc):
        for name, a in (("prob", prob), ("loc_pred", loc)):
            assert self.net.blobs[name].shape == a.shape, (name, self.net.blobs[name].shape, a.shape)
            self.net.blobs[name].data[...] = a

    def plant(self, prob, loc):
        """The net forwarded once at the maps' size, then its `prob` and `loc_pred` overwritten."""
        n, _, h, w = prob.shape
        self.net.blobs["data"].reshape(n, 3, h * STRIDE, w * STRIDE)
        self.net.reshape()
        self.net.blobs["data"].data[...] = 0
        self.net.forward()
        self.write(prob, loc)

    def fused(self):
        return self.grp.fuse_maps((1.0,), 0, want=MAPS)


@pytest.fixture(scope="module", params=["f32", "f16", "bf16"])
def reader(request, gpu_caffe):
    return Reader(gpu_caffe, request.param)


_answers = {}


def _answer(key, make):
    """The float64 answers, computed once per process and shared by the element types."""
    if key not in _answers:
        _answers[key] = make()
    return _answers[key]


def _check_poses(got, want, scale, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got[:, 2], want[:, 2]), what
    for b in range(len(want)):
        rows, cols = ep.pose_cells(got[b], scale)
        rrows, rcols = ep.pose_cells(want[b], scale)
        assert np.array_equal(rows, rrows) and np.array_equal(cols, rcols), (what, b, rows, rrows, cols, rcols)
    assert np.allclose(got, want, rtol=0, atol=1e-9), what


def _check_parts(got, want, what):
    (counts, dets), (rcounts, rdets) = got, want
    assert np.array_equal(counts, rcounts), (what, counts, rcounts)
    assert dets.shape == rdets.shape and not np.isnan(dets).any(), what
    for k, name in ((2, "score"), (3, "row"), (4, "col")):
        assert np.array_equal(dets[..., k], rdets[..., k]), (what, name)
    assert np.allclose(dets[..., :2], rdets[..., :2], rtol=0, atol=1e-9), what


def _both_decoders(rd, key, prob, loc, scales=(1.0, 0.75)):
    """Net.decode_pose and NetGroup.decode_pose (whose fused maps are the planted ones) against pose_from_maps."""
    for scale in scales:
        want = _answer(("pose", key, scale), lambda: MC.poses(prob, loc, scale))
        _check_poses(rd.net.decode_pose(scale), want, scale, (rd.kind, key, "Net.decode_pose", scale))
        _check_poses(rd.grp.decode_pose((scale,), 0), want, scale, (rd.kind, key, "NetGroup.decode_pose", scale))


def _both_selectors(rd, key, prob, loc, thr, radius, md, scale=1.0, twice=False):
    """Net.detect_parts and NetGroup.detect_parts against nms_candidates; twice: the same bits from a second call."""
    want = _answer(("parts", key, thr, radius, md, scale), lambda: MC.parts(prob, loc, scale, thr, radius, md))
    for name, call in (("Net.detect_parts", lambda: rd.net.detect_parts(scale, thr, radius, md)),
                       ("NetGroup.detect_parts", lambda: rd.grp.detect_parts((scale,), 0, thr, radius, md))):
        got = call()
        _check_parts(got, want, (rd.kind, key, name, thr, radius, md))
        if twice:
            again = call()
            assert np.array_equal(got[0], again[0]) and np.array_equal(got[1].view(np.uint64), again[1].view(np.uint64)), (rd.kind, key, name, md)


def _fused_is_planted(rd, prob, loc):
    f = rd.fused()
    assert f["prob"].dtype == np.float32 and np.array_equal(f["prob"], prob) and np.array_equal(f["loc_pred"], loc), rd.kind


def test_first_maximum_on_ties_and_trip_boundaries(reader):
    """19 x 29 = 551 cells, batch 2: every joint's pattern of map_reader_cases.FIRST_PATTERNS through the scan's three trips and the LDS
    tree.  The answer is the lowest cell at the maximum, cell 0 for a plateau and for an all-zero map."""
    case = MC.first_max_case()
    prob, loc = case["prob"], case["loc"]
    reader.plant(prob, loc)
    _fused_is_planted(reader, prob, loc)
    _both_decoders(reader, "first", prob, loc)
    got = reader.net.decode_pose(1.0)
    w = prob.shape[3]
    for b in range(2):
        rows, cols = ep.pose_cells(got[b], 1.0)
        assert [int(r) * w + int(c) for r, c in zip(rows, cols)] == [cells[0] for cells in case["maxima"][b]], (reader.kind, b)
    # the same maps through the window test: plateaus and pairs under the lower-cell rule
    for radius in (1, 2):
        _both_selectors(reader, "first", prob, loc, MC.THR, radius, 8)


@pytest.mark.parametrize("built_for", MC.WINDOW_RADII)
def test_nms_windows_on_edges_ties_and_the_threshold(reader, built_for):
    """16 x 23 maps: corners, edges, an equal pair inside one window and one radius + 1 apart, a score at the threshold and one step
    below, plateaus, and level maps that tie all over; each map at both radii (at the other radius the pairs fall on the other side of
    the window's edge), with max_det below and above the counts."""
    case = MC.window_case(built_for)
    prob, loc = case["prob"], case["loc"]
    reader.plant(prob, loc)
    _fused_is_planted(reader, prob, loc)
    for radius in MC.WINDOW_RADII:
        for md in (4, 32):
            _both_selectors(reader, ("window", built_for), prob, loc, MC.THR, radius, md, scale=1.0 if md == 4 else 0.75)
    got = reader.net.detect_parts(1.0, MC.THR, built_for, 32)
    w = prob.shape[3]
    for j, cells in case["survivors"].items():
        assert [int(r) * w + int(c) for r, c in got[1][0, j, :got[0][0, j], 3:]] == cells, (reader.kind, built_for, j)
    _both_decoders(reader, ("window", built_for), prob, loc, scales=(1.0,))


def test_candidate_counts_on_the_sort_boundaries(reader):
    """64 x 65 = 4160 cells, radius 0, one joint per count of map_reader_cases.COUNTS: 0, 1, 257 (the zero-key padding of the bitonic
    sort), 4096 (the LDS sort) against 4097 (the spill path) and their neighbours, four distinct scores for all of them.  max_det 1, 96,
    300 and 4096: below, at (4096) and above every count that detect_parts' limit of 4096 lets it be above.  Every call twice."""
    case = MC.counts_case()
    prob, loc = case["prob"], case["loc"]
    reader.plant(prob, loc)
    _fused_is_planted(reader, prob, loc)
    for md in (1, 96, 300, 4096):
        _both_selectors(reader, "counts", prob, loc, MC.THR, 0, md, twice=True)
    counts, _ = reader.net.detect_parts(1.0, MC.THR, 0, 4096)
    assert tuple(counts[0]) == tuple(min(n, 4096) for n in MC.COUNTS)
    _both_decoders(reader, "counts", prob, loc, scales=(1.0,))  # hundreds of cells at the maximum 255 / 256


def test_both_signs_of_zero_at_threshold_zero(reader):
    """+0.0, -0.0, a float16-denormal-sized score (2^-16 on a float16 net, 2^-20 elsewhere) and ordinary scores at threshold 0, max_det
    below the number of candidates: a zero of either sign sorts below every positive score and among the zeros by cell.  The group
    reads its fused float32 maps, where (1 - 0) * -0.0 + 0 * x has lost the sign: its answer is the restatement's on those maps."""
    exp = -16 if reader.kind == "f16" else -20
    case = MC.zeros_case(exp)
    prob, loc = case["prob"], case["loc"]
    reader.plant(prob, loc)
    assert np.array_equal(np.signbit(reader.net.blobs["prob"].data), np.signbit(prob))  # -0.0 is in the net
    fused = reader.fused()
    assert np.array_equal(fused["prob"], prob) and np.array_equal(fused["loc_pred"], loc)
    for radius in (0, 1):
        want = _answer(("zeros", exp, radius), lambda: MC.parts(prob, loc, 1.0, 0.0, radius, MC.ZERO_MAX_DET))
        _check_parts(reader.net.detect_parts(1.0, 0.0, radius, MC.ZERO_MAX_DET), want, (reader.kind, "zeros", "Net.detect_parts", radius))
        mine = MC.parts(fused["prob"], fused["loc_pred"], 1.0, 0.0, radius, MC.ZERO_MAX_DET)
        _check_parts(reader.grp.detect_parts((1.0,), 0, 0.0, radius, MC.ZERO_MAX_DET), mine, (reader.kind, "zeros", "NetGroup.detect_parts", radius))
        _check_parts(mine, want, "the restatement on the fused maps")
    _both_decoders(reader, ("zeros", exp), prob, loc, scales=(1.0,))


def test_nan_cells_are_never_selected_and_never_suppress(reader):
    """NaN beside maxima.  The member's own maps hold the planted NaN cells; the group's fused maps hold more (0 * NaN of the bilinear
    sample's unused corners), so the group is held to the restatement on the maps fuse_maps returns."""
    case = MC.nan_case()
    prob, loc = case["prob"], case["loc"]
    reader.plant(prob, loc)
    assert np.array_equal(np.isnan(reader.net.blobs["prob"].data), np.isnan(prob))
    fused = reader.fused()
    assert np.isnan(fused["prob"][np.isnan(prob)]).all() and np.array_equal(fused["prob"][~np.isnan(fused["prob"])], prob[~np.isnan(fused["prob"])])
    for radius in (1, 2):
        want = _answer(("nan", radius), lambda: MC.parts(prob, loc, 1.0, MC.THR, radius, 32))
        _check_parts(reader.net.detect_parts(1.0, MC.THR, radius, 32), want, (reader.kind, "NaN", "Net.detect_parts", radius))
        mine = MC.parts(fused["prob"], fused["loc_pred"], 1.0, MC.THR, radius, 32)
        _check_parts(reader.grp.detect_parts((1.0,), 0, MC.THR, radius, 32), mine, (reader.kind, "NaN", "NetGroup.detect_parts", radius))


def test_restricted_decode_with_the_global_maximum_outside_the_box(reader, gpu_caffe):
    """NetGroup.forward_boxes of five boxes on a one-member group (valid cells 13 x 29 full width, 18 x 19 narrow, 1 x 1, the whole
    20 x 29 map, 10 x 3 at scale 0.5), the member's maps then overwritten so that every joint's global maximum and ties with the
    region's maximum lie OUTSIDE the region, ties inside it and its maximum at its last cell; then decode_boxes."""
    case = MC.restricted_case()
    prob, loc = case["prob"], case["loc"]
    img = np.random.RandomState(9).randint(0, 256, MC.BOX_IMAGE_HW + (3,)).astype(np.uint8)
    reader.grp.forward_boxes(img, MC.BOXES, (1.0,), MC.BOX_SCALES, canvas=MC.BOX_CANVAS, want=(), pose=False)
    reader.write(prob, loc)
    got = reader.grp.decode_boxes((1.0,), 0, want=MAPS)
    assert np.array_equal(got["prob"], prob) and np.array_equal(got["loc_pred"], loc)
    want = _answer("boxes", lambda: MC.box_poses(prob, loc))
    H, W = prob.shape[2:]
    pose = got["pose"]
    assert pose.shape == want.shape == (len(MC.BOXES), 5, MC.J)
    assert np.array_equal(pose[:, 2], want[:, 2]), reader.kind
    for i, (box, s, (rows_own, cols_own)) in enumerate(zip(MC.BOXES, MC.BOX_SCALES, MC.BOX_REGIONS)):
        shift = np.array([[box[0]], [box[1]], [0], [0], [0]])
        rows, cols = ep.pose_cells(pose[i] - shift, s)
        rrows, rcols = ep.pose_cells(want[i] - shift, s)
        assert np.array_equal(rows, rrows) and np.array_equal(cols, rcols), (reader.kind, i, rows, rrows, cols, rcols)
        assert (rows < rows_own).all() and (cols < cols_own).all()
        assert [int(r) * W + int(c) for r, c in zip(rows, cols)] == [cells[0] for cells in case["inside"][i]], (reader.kind, i)
    assert np.allclose(pose, want, rtol=0, atol=1e-9), reader.kind
    assert np.array_equal(reader.grp.decode_boxes((1.0,), 0)["pose"], pose)

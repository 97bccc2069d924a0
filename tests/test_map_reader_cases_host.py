"""The crafted maps of tests/map_reader_cases.py hold their own preconditions (no GPU): what tests/test_gpu_map_readers.py runs through
the device really is a tie, a boundary count, a maximum outside the box — and really is what a 16-bit net reads."""
import numpy as np
import pytest

import map_reader_cases as MC
from oracle.multiperson import nms_candidates


def _all_cases():
    yield "first maximum", MC.first_max_case()
    for r in MC.WINDOW_RADII:
        yield "windows, radius %d" % r, MC.window_case(r)
    yield "counts", MC.counts_case()
    yield "zeros, 2^-20", MC.zeros_case(-20)
    yield "zeros, 2^-16", MC.zeros_case(-16)
    yield "NaN", MC.nan_case()
    yield "restricted decode", MC.restricted_case()


def test_every_value_is_exact_in_float16_and_bfloat16():
    for name, case in _all_cases():
        for k in ("prob", "loc"):
            a = case[k]
            assert a.dtype == np.float32 and not a.flags.writeable, (name, k)
            assert MC.rounds_to_itself(a), (name, k)
        special = name.startswith("zeros") or name == "NaN"
        p = case["prob"][~np.isnan(case["prob"])]
        if not special:
            assert np.array_equal(p * 256, np.round(p * 256)) and p.min() >= 0 and p.max() <= 1, name
        assert np.array_equal(case["loc"] * 8, np.round(case["loc"] * 8)) and np.abs(case["loc"]).max() <= 1, name
    # (the helper itself tells a value that does not survive)
    assert not MC.rounds_to_itself(np.array([1.0 / 3], np.float32)) and not MC.rounds_to_itself(np.array([257.0 / 256], np.float32))
    assert not MC.rounds_to_itself(np.array([2.0 ** -30], np.float32))


def test_first_maximum_patterns_are_what_they_say():
    case = MC.first_max_case()
    h, w = MC.FIRST_HW
    assert h * w > 512 and (h * w) % 256 and case["prob"].shape == (2, MC.J, h, w)
    assert [n for n, _ in MC.FIRST_PATTERNS[0]] != [n for n, _ in MC.FIRST_PATTERNS[1]]
    want = set(["plateau over the whole map", "two maxima one thread apart", "two maxima one trip apart", "the maximum at the last cell",
                "the maximum at cell 255", "the maximum at cell 256", "an all-zero map"])
    for b in range(2):
        assert all(any(w in name for name in case["what"][b]) for w in want), b
        for j in range(MC.J):
            flat, cells, what = case["prob"][b, j].reshape(-1), case["maxima"][b][j], case["what"][b][j]
            assert np.array_equal(np.flatnonzero(flat == flat.max()), cells), (b, j, what)
            assert int(flat.argmax()) == cells[0]
            if "maxima" in what or "plateau" in what or "all-zero" in what:
                assert len(cells) >= 2, what
            if "all-zero" in what:
                assert not flat.any()
            if "one thread apart" in what:
                assert cells[1] == cells[0] + 1
            if "one trip apart" in what:
                assert cells[1] == cells[0] + 256
            if "of one thread" in what:
                assert len(set(c % 256 for c in cells)) == 1 and len(set(c // 256 for c in cells)) == len(cells)
            if "lower LDS half" in what:  # the LDS tree meets the larger index in the half it keeps, the smaller one in the half it folds in
                assert cells[0] % 256 >= 128 > cells[1] % 256
    assert case["maxima"][0][5] == (h * w - 1,) and case["maxima"][0][6] == (255,) and case["maxima"][0][7] == (256,)


@pytest.mark.parametrize("radius", MC.WINDOW_RADII)
def test_window_case_survivors(radius):
    case = MC.window_case(radius)
    h, w = MC.WINDOW_HW
    prob, loc = case["prob"][0], case["loc"][0]
    counts, dets = nms_candidates(prob, loc, 1.0, MC.THR, radius, 32)
    for j, cells in case["survivors"].items():
        got = [int(r) * w + int(c) for r, c in dets[j, :counts[j], 3:]]
        assert got == cells, (radius, j, got, cells)
    # corners and edges are there, the pair inside one window lost its second cell, the pair radius + 1 apart kept both
    assert set(case["survivors"][0]) == {0, w - 1, (h - 1) * w, h * w - 1}
    assert prob[2, 3, 3] == prob[2, 3, 3 + radius] and counts[2] == 2 and counts[3] == 6
    assert prob[3, 3, 3] == prob[3, 3, 4 + radius] and prob[3, 9, 14] == prob[3, 10 + radius, 14]
    # exactly at the threshold, and one step below
    assert prob[4, 4, 4] == np.float32(MC.THR) and prob[4, 4, 12] == np.float32(MC.THR - 1.0 / 256) and counts[4] == 2
    # the level maps tie all over: fewer distinct scores than candidates
    for j in range(7, MC.J):
        assert counts[j] > len(np.unique(dets[j, :counts[j], 2]))


def test_counts_are_the_boundary_numbers():
    prob = MC.counts_case()["prob"][0]
    assert prob.shape[1] * prob.shape[2] >= 4160
    assert tuple((prob[j] >= MC.THR).sum() for j in range(MC.J)) == MC.COUNTS
    assert set((0, 1, 257, 4096, 4097)) <= set(MC.COUNTS)
    for j, n in enumerate(MC.COUNTS):
        if n > 4:
            assert len(np.unique(prob[j][prob[j] >= MC.THR])) <= 4 < n  # equal scores everywhere
        assert n == prob[j].size or (prob[j] == np.float32(127 / 256.0)).any()  # one step below the threshold is there and is not counted


@pytest.mark.parametrize("tiny_exp", [-20, -16])
def test_zeros_case_mixes_both_zeros(tiny_exp):
    prob = MC.zeros_case(tiny_exp)["prob"][0]
    tiny = np.float32(2.0) ** tiny_exp
    assert 0 < tiny < np.float32(2.0) ** -14  # below float16's smallest normal
    for j in range(MC.J):
        p = prob[j].reshape(-1)
        neg, pos = (p == 0) & np.signbit(p), (p == 0) & ~np.signbit(p)
        assert neg.sum() >= 20 and pos.sum() >= 10 and (p == tiny).sum() == 1 and (p >= 0).all()
        assert (p > 0).sum() < MC.ZERO_MAX_DET < p.size  # zeros are listed, and not all of them
        listed = np.flatnonzero(p == 0)[:MC.ZERO_MAX_DET - (p > 0).sum()]
        assert neg[listed].any() and pos[listed].any()  # of both signs
    # the restatement orders -0.0 with +0.0: by cell
    counts, dets = nms_candidates(prob, MC.zeros_case(tiny_exp)["loc"][0], 1.0, 0.0, 0, MC.ZERO_MAX_DET)
    assert (counts == MC.ZERO_MAX_DET).all()
    for j in range(MC.J):
        zeros = dets[j][dets[j][:, 2] == 0]
        cells = zeros[:, 3] * prob.shape[2] + zeros[:, 4]
        assert len(zeros) >= 6 and (np.diff(cells) > 0).all() and (np.diff(dets[j][:, 2]) <= 0).all()


def test_nan_case_has_nan_beside_its_maxima():
    prob = MC.nan_case()["prob"][0]
    assert np.isnan(prob[0, 4, 4]) and np.isnan(prob[0, 3, 5]) and prob[0, 4, 5] == prob[0][~np.isnan(prob[0])].max()
    assert all(np.isnan(prob[j]).sum() >= 1 for j in range(MC.J))
    counts, dets = nms_candidates(prob, MC.nan_case()["loc"][0], 1.0, MC.THR, 1, 32)
    assert not np.isnan(dets).any() and counts[0] == 1 and counts[1] == 1
    assert counts[2] == 2  # two cells apart at radius 1, NaN between them: both stay


def test_restricted_case_regions():
    from pose.estimate_pose import crop_canvas_size

    case = MC.restricted_case()
    H, W = MC.BOX_CANVAS[0] // 8, MC.BOX_CANVAS[1] // 8
    assert case["prob"].shape == (len(MC.BOXES), MC.J, H, W)
    kinds = set()
    for i, ((x0, y0, x1, y1), s, (rows, cols)) in enumerate(zip(MC.BOXES, MC.BOX_SCALES, MC.BOX_REGIONS)):
        assert 0 <= x0 < x1 <= MC.BOX_IMAGE_HW[1] and 0 <= y0 < y1 <= MC.BOX_IMAGE_HW[0]
        oh, ow = crop_canvas_size(y1 - y0, x1 - x0, s)
        assert (oh // 8, ow // 8) == (rows, cols) and rows <= H and cols <= W
        kinds.add(("full width" if cols == W else "narrow") if rows < H else "to the canvas edge")
        if rows * cols == 1:
            kinds.add("1x1")
        for j in range(MC.J):
            m = case["prob"][i, j]
            inside, cells = m[:rows, :cols], case["inside"][i][j]
            assert [int(r) * W + int(c) for r, c in zip(*np.nonzero(inside == inside.max()))] == cells
            if rows * cols > 1 and (i + j) % 6 != 2:
                assert len(cells) >= 2, (i, j)  # a tie inside the region
            if (i + j) % 6 in (2, 3):
                assert cells[-1] == (rows - 1) * W + cols - 1  # the region's last cell
            if rows < H or cols < W:
                outside = m.copy()
                outside[:rows, :cols] = -1
                assert outside.max() > inside.max(), (i, j)  # the global maximum lies outside, strictly
                assert int(m.argmax()) not in cells and (outside == inside.max()).any()  # and so do ties with the region's maximum
    assert kinds == {"full width", "narrow", "to the canvas edge", "1x1"}
    # the narrow region's walk leaves its first trip, and one of its tie pairs is 256 walk steps apart
    rows, cols = MC.BOX_REGIONS[1]
    assert cols < W and rows * cols > 256
    j = [j for j in range(MC.J) if (1 + j) % 6 == 1][0]
    a, b = case["inside"][1][j]
    assert (b // W) * cols + b % W - ((a // W) * cols + a % W) == 256

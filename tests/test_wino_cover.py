"""CPU: the cover planner of the mixed float32 Winograd forms (wino_f32.hip wino_plan_cover, through dc_wino_cover): one straight cut of the
tile grid, 4 x 8-tile blocks in front of it and 5 x 6-tile blocks behind it.  For every grid up to 48 x 48 tiles the block slots the kernel
would run cover every tile exactly once, no block is empty, the count is the least any single straight cut allows, and the forms are
offered to the per-shape timing exactly where that count is strictly below both pure covers."""
import pytest

N = 48
A_BTY, A_BTX, B_BTY, B_BTX = 4, 8, 5, 6


def _ceil(a, b):
    return -(-a // b)


def _pure(ty, tx, bty, btx):
    return _ceil(ty, bty) * _ceil(tx, btx)


def _best_single_cut(ty, tx):
    """Fewest blocks over every straight cut at every position, either geometry on either side (an enumeration of its own, not the planner's)."""
    best = min(_pure(ty, tx, A_BTY, A_BTX), _pure(ty, tx, B_BTY, B_BTX))
    for first, second in (((A_BTY, A_BTX), (B_BTY, B_BTX)), ((B_BTY, B_BTX), (A_BTY, A_BTX))):
        for cut in range(1, ty):
            best = min(best, _pure(cut, tx, *first) + _pure(ty - cut, tx, *second))
        for cut in range(1, tx):
            best = min(best, _pure(ty, cut, *first) + _pure(ty, tx - cut, *second))
    return best


@pytest.fixture(scope="module")
def covers():
    import caffe

    return {(ty, tx): caffe.wino_cover(ty, tx) for ty in range(1, N + 1) for tx in range(1, N + 1)}


def test_the_regions_partition_every_grid(covers):
    for (ty, tx), c in covers.items():
        seen = [[0] * tx for _ in range(ty)]
        regions = (((0, 0), (c["a_nby"], c["a_nbx"]), (A_BTY, A_BTX)), ((c["b_ty0"], c["b_tx0"]), (c["b_nby"], c["b_nbx"]), (B_BTY, B_BTX)))
        assert c["a_nby"] * c["a_nbx"] == c["na"] and c["b_nby"] * c["b_nbx"] == c["nb"] and c["na"] + c["nb"] == c["blocks"], (ty, tx, c)
        for (y0, x0), (nby, nbx), (bty, btx) in regions:
            for by in range(nby):
                for bx in range(nbx):
                    tiles = 0
                    for y in range(y0 + by * bty, min(y0 + (by + 1) * bty, ty)):  # (the kernel keeps a slot whose tile lies inside the grid)
                        for x in range(x0 + bx * btx, min(x0 + (bx + 1) * btx, tx)):
                            seen[y][x] += 1
                            tiles += 1
                    assert tiles > 0, "a block wholly outside the grid: %r" % ((ty, tx, c),)
        assert all(v == 1 for row in seen for v in row), (ty, tx, c)
        # region A ends on the cut: in front of it when horizontal (rows), left of it when vertical (columns)
        if c["na"] and c["nb"]:
            assert (c["b_ty0"], c["b_tx0"]) == ((0, c["cut"]) if c["vertical"] else (c["cut"], 0)), (ty, tx, c)


def test_block_counts_are_minimal_and_no_worse_than_the_pure_covers(covers):
    import caffe

    for (ty, tx), c in covers.items():
        p48, p56 = _pure(ty, tx, A_BTY, A_BTX), _pure(ty, tx, B_BTY, B_BTX)
        assert c["blocks"] <= p48 and c["blocks"] <= p56, (ty, tx, c)
        assert c["blocks"] == _best_single_cut(ty, tx), (ty, tx, c)
        assert bool(c["offered"]) == (c["blocks"] < p48 and c["blocks"] < p56), (ty, tx, c)
        # ties: a pure cover before a cut one (9 x 12 stays four 5 x 6 blocks although 2 + 2 would do), 4 x 8 before 5 x 6: fewest 5 x 6 blocks
        if c["blocks"] == p48:
            assert c["nb"] == 0, (ty, tx, c)
        elif c["blocks"] == p56:
            assert c["na"] == 0, (ty, tx, c)
    for tile in ("wino_f23_mix", "wino_f23_mix_w16"):
        assert all(caffe.wino_blocks(tile, ty, tx) == c["blocks"] for (ty, tx), c in list(covers.items())[::37])


@pytest.mark.parametrize("grid,blocks,na,nb,vertical,offered", [
    ((17, 23), 13, 9, 4, 0, 1),      # res4 at 544x736: rows 0-11 as 3 x 3 blocks of 4 x 8, rows 12-16 as 1 x 4 of 5 x 6 (15 / 16 pure)
    ((34, 46), 52, 45, 7, 1, 1),     # res3 (54 / 56 pure): the horizontal cut at row 24 needs 52 too, with 16 blocks of 5 x 6 against 7
    ((68, 92), 198, 170, 28, 1, 1),  # res2, by a vertical cut (204 / 224 pure)
    ((9, 12), 4, 0, 4, 0, 0),        # a phase image of the dilated res5 layers: pure 5 x 6
    ((20, 14), 9, 5, 4, 1, 1),       # a vertical cut (10 / 12 pure)
    ((9, 13), 5, 3, 2, 1, 1),        # the smallest grid with a vertical cut (6 / 6 pure)
    ((14, 27), 14, 8, 6, 1, 1),      # ... with two block columns on either side of it (16 / 15 pure)
    ((1, 1), 1, 1, 0, 0, 0),
])
def test_the_covers_of_the_benchmark_shapes(covers, grid, blocks, na, nb, vertical, offered):
    c = covers[grid] if grid in covers else __import__("caffe").wino_cover(*grid)
    assert (c["blocks"], c["na"], c["nb"], c["offered"]) == (blocks, na, nb, offered), c
    if na and nb:
        assert c["vertical"] == vertical, c


def test_the_smallest_vertical_cut(covers):
    """tests/test_gpu_winograd_mixed.py runs 9 x 13 tiles as its smallest vertical-cut case: no grid of fewer tiles has an offered cover
    that is cut vertically (and none at all has an offered cover of fewer than five blocks)."""
    vertical = [(ty * tx, ty, tx) for (ty, tx), c in covers.items() if c["offered"] and c["vertical"]]
    assert min(vertical) == (117, 9, 13), min(vertical)
    assert min(c["blocks"] for c in covers.values() if c["offered"]) == 5


@pytest.mark.parametrize("tiles,images,cout,want", [
    ((17, 23), 1, 256, 1),   # res4 at 544x736: 15 x 16 = 240 workgroups on 4 x 8 blocks
    ((34, 46), 1, 128, 1),   # res3: 432
    ((68, 92), 1, 64, 1),    # res2: 816
    ((9, 12), 4, 512, 0),    # res5, four phase images: the cover is the pure 5 x 6 one
    ((9, 13), 1, 64, 0),     # res2 of a 72 x 104 image: 5 blocks against 6, but 24 workgroups: nobody waits for the four it would free
    ((9, 13), 1, 320, 0),    # 120 workgroups
    ((9, 13), 1, 352, 1),    # 132: half the CUs
    ((9, 13), 6, 64, 1),     # ... by the batch: 144
])
def test_the_forms_are_offered_to_launches_of_half_the_chip_or_more(tiles, images, cout, want):
    """ConvForm::offered of the mixed forms: a cover with strictly fewer blocks than both pure ones AND a launch that, on 4 x 8 blocks, has
    at least 128 workgroups (half of the 256 CUs)."""
    import caffe

    assert caffe.wino_mix_offered(*tiles, images, cout) == want
    if want:
        assert caffe.wino_cover(*tiles)["offered"] == 1


def test_bad_arguments():
    import caffe

    assert caffe.wino_cover(0, 5) is None and caffe.wino_cover(5, -1) is None
    assert caffe.wino_mix_offered(0, 5, 1, 64) == -1 and caffe.wino_mix_offered(9, 13, 0, 64) == -1

"""CPU: the block geometries of the float32 Winograd kernel (wino_f32.hip, WinoGeom): how many tile blocks a form needs for a tile grid
(dc_wino_blocks: what decides where the 5 x 6 forms enter the per-shape timing), and the LDS layout of the 5 x 6 block's 12 x 14 staged
pixels against the bank model of tools/lds_bank_model.py: every patch-row read (ds_read_b128) of both fragments stays at 4 LDS cycles,
and three stages stay within half of a CU's LDS (two workgroups per CU)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import lds_bank_model as M  # noqa: E402


def _geometries():
    """{name: (fragment rows, fragment columns, side by side, row pitch)} as wino_f32.hip instantiates them."""
    src = open(os.path.join(ROOT, "deepcut-cnn_amd", "csrc", "wino_f32.hip")).read()
    found = re.findall(r"using (WinoG\d+) = WinoGeom<(\d+), (\d+), (true|false), (\d+)>;", src)
    g = {n: (int(fr), int(fc), side == "true", int(p)) for n, fr, fc, side, p in found}
    # the default block is spelled with the constants tests/test_lds_layout_model.py reads
    assert "using WinoG48 = WinoGeom<WBTY / 2, WBTX, false, WPITCH>;" in src
    bty, btx = map(int, re.search(r"constexpr int WBTY = (\d+), WBTX = (\d+),", src).groups())
    g["WinoG48"] = (bty // 2, btx, False, int(re.search(r"constexpr int WPITCH = (\d+);", src).group(1)))
    return g


@pytest.mark.parametrize("grid,want56,want48", [((9, 12), 4, 6), ((17, 23), 16, 15), ((34, 46), 56, 54), ((68, 92), 224, 204), ((1, 1), 1, 1),
                                                ((5, 6), 1, 2), ((6, 7), 4, 2), ((1, 13), 3, 2), ((11, 1), 3, 3)])
def test_block_counts(grid, want56, want48):
    import caffe

    for tile in ("wino_f23_5x6", "wino_f23_5x6_w16"):
        assert caffe.wino_blocks(tile, *grid) == want56, (tile, grid)
    for tile in ("wino_f23", "wino_f23_w16"):
        assert caffe.wino_blocks(tile, *grid) == want48, (tile, grid)


def test_block_counts_of_other_names():
    import caffe

    assert caffe.wino_blocks("ws1x1f", 9, 12) == -1 and caffe.wino_blocks("no_such_tile", 9, 12) == -1
    assert caffe.wino_blocks("wino_f23_5x6", 0, 12) == -1


def test_the_source_names_both_geometries():
    g = _geometries()
    assert g["WinoG48"] == (2, 8, False, 672) and g["WinoG56"][:3] == (5, 3, True)


def test_the_5x6_block_reads_its_patch_rows_without_conflicts_and_fits_twice_per_cu():
    fr, fc, side, pitch = _geometries()["WinoG56"]
    rows, cols = 2 * fr + 2, 2 * (2 * fc) + 2  # staged pixels: 12 x 14
    assert (rows, cols) == (12, 14) and fr * fc <= 16
    assert pitch >= cols * 36 and pitch % 4 == 0
    assert 2 * 3 * (rows * pitch + 8) * 4 <= 160 * 1024  # ring of three stages (+ the dump slot), two workgroups per CU
    for tf in (0, 1):
        for row0 in range(4):
            addr = M.wino_geom_read(fr, fc, side, pitch, tf, row0)
            assert M.ds_read_b128_cycles(addr) == 4, (tf, row0)
            assert max(addr) + 4 + 3 * 36 + 16 <= rows * pitch  # the four pixels x two channel halves a lane reads stay inside the stage
    # what the pitch is for: a plain 512 or the tightest 504 collide
    assert M.wino_geom_cycles(fr, fc, side, 512) > 4 and M.wino_geom_cycles(fr, fc, side, 504) > 4


def test_the_model_agrees_on_the_4x8_block():
    fr, fc, side, pitch = _geometries()["WinoG48"]
    assert M.wino_geom_cycles(fr, fc, side, pitch) == 4 == M.wino_layout_cycles(36, pitch)
    for row0 in range(4):  # the geometry form of the read is the read tests/test_lds_layout_model.py models
        assert M.wino_geom_read(fr, fc, side, pitch, 0, row0) == M.wino_patch_row_read(36, pitch, row0)


def test_the_staging_stores_of_both_blocks_are_conflict_free():
    """A ds_write_b128 is served in groups of eight consecutive lanes on 32 banks; eight consecutive staging threads write the eight channel
    quads of one pixel, 32 consecutive floats, whatever the row pitch.  (The threads past the block share two dump slots: broadcast-like
    duplicates, not distinct addresses.)"""
    for name, nth in (("WinoG48", 512), ("WinoG56", 512), ("WinoG48", 1024), ("WinoG56", 1024)):
        fr, fc, side, pitch = _geometries()[name]
        rows, cols = 2 * (fr if side else 2 * fr) + 2, 2 * (2 * fc if side else fc) + 2
        nld = -(-rows * cols * 8 // nth)
        for q in range(nld):
            for wave in range(nth // 64):
                assert M.ds_write_b128_cycles(M.wino_stage_store(rows, cols, pitch, wave, q, nth)) == 8, (name, nth, q, wave)

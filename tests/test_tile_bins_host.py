"""The overlays' tile binner (deepcut-cnn_amd/csrc/tile_bins.h, shared by dc_draw_people and dc_redact_people) against brute force,
under AddressSanitizer + UBSan, CPU only (tools/probes/tile_bins_check.cpp, a program of its own run as a child process): seeded random
discs and capsules in three 70 x 45 frames — 3 x 2 tiles with a partial last column and row, a frame that gets nothing, primitives
wholly outside, primitives over every tile, radius 1.  A tile must list a primitive exactly when it holds a pixel whose centre lies in
the primitive's box grown by its radius; indices ascend; tiles come by frame, row, column and none is empty; the counts sum to the
index length; a frame is touched exactly when it has a tile; what lies wholly outside is not kept."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tile_bins") / "tile_bins_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "deepcut-cnn_amd", "csrc"), os.path.join(ROOT, "tools", "probes", "tile_bins_check.cpp"),
                        "-o", exe], capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("no sanitizer runtime in this image")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_bins_match_brute_force(harness, seed):
    r = subprocess.run([harness, str(seed)], capture_output=True, text=True, timeout=120, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "OK" in r.stdout

"""CPU: the NV12 conversion rule (include/deepcut_hip.h, dc_frame) — its coefficient integers, its distance from the real-valued matrix
and from Pillow over all 2^24 (Y, Cb, Cr) triples, `caffe.Frame.to_bgr` against the restatement in tests/nv12_ref.py, and what
`caffe.Frame` refuses without a device.

The bound of one level is derived, not measured: each coefficient is within 2^-17 of the real one and multiplies a value of at most
255, so the fixed-point sum is within 3 * 255 * 2^-17 < 0.006 of the real-valued one before both are rounded — the two roundings can
fall on either side of a half, never further apart than one level."""
import numpy as np
import pytest

import nv12_ref as NR


def _triples(y_lo, y_hi):
    """Every (Y, Cb, Cr) with y_lo <= Y < y_hi, as three flat int32 arrays."""
    y, cb, cr = np.meshgrid(np.arange(y_lo, y_hi, dtype=np.int32), np.arange(256, dtype=np.int32), np.arange(256, dtype=np.int32),
                            indexing="ij")
    return y.ravel(), cb.ravel(), cr.ravel()


def test_coefficient_integers():
    assert NR.coefficients("bt601", "limited") == (76309, 104597, 132201, -25675, -53279)
    assert NR.coefficients("bt709", "limited") == (76309, 117489, 138438, -13975, -34925)
    assert NR.coefficients("bt601", "full") == (65536, 91881, 116130, -22553, -46802)


def test_product_coefficients_are_the_restatement():
    import caffe

    for m in NR.MATRICES:
        for r in NR.RANGES:
            assert caffe.csc_coefficients(m, r) == NR.coefficients(m, r) + (NR.scales(r)[0],)


@pytest.mark.parametrize("matrix", NR.MATRICES)
@pytest.mark.parametrize("range_", NR.RANGES)
def test_within_one_level_of_the_real_valued_matrix_on_all_triples(matrix, range_):
    worst = 0
    for y0 in range(0, 256, 32):
        t = _triples(y0, y0 + 32)
        got, want = NR.convert(*t, matrix, range_), NR.real_valued(*t, matrix, range_)
        worst = max(worst, max(int(np.abs(g - w).max()) for g, w in zip(got, want)))
    print("%s %s: max |rule - real-valued| = %d level(s) over 2^24 triples" % (matrix, range_, worst))
    assert worst <= 1


def test_full_range_bt601_within_one_level_of_pillow_on_all_triples():
    from PIL import Image

    worst = 0
    for y0 in range(0, 256, 64):
        t = _triples(y0, y0 + 64)
        planes = [Image.fromarray(v.astype(np.uint8).reshape(4096, 1024)) for v in t]
        rgb = np.asarray(Image.merge("YCbCr", planes).convert("RGB")).reshape(-1, 3).astype(np.int32)
        got = NR.convert(*t, "bt601", "full")
        worst = max(worst, max(int(np.abs(got[k] - rgb[:, k]).max()) for k in range(3)))
    print("bt601 full: max |rule - Pillow| = %d level(s) over 2^24 triples" % worst)
    assert worst <= 1


def _planes(h, w, seed, pitch_y=None, pitch_uv=None):
    """Random NV12 planes of an h x w frame as views into pitched buffers whose padding is 0xFF."""
    rs = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    py, puv = pitch_y or w, pitch_uv or 2 * cw
    ybuf, uvbuf = np.full((h, py), 0xFF, np.uint8), np.full((ch, puv), 0xFF, np.uint8)
    ybuf[:, :w] = rs.randint(0, 256, (h, w))
    uvbuf[:, : 2 * cw] = rs.randint(0, 256, (ch, 2 * cw))
    return ybuf[:, :w], np.lib.stride_tricks.as_strided(uvbuf, (ch, cw, 2), (puv, 2, 1))


@pytest.mark.parametrize("hw", [(37, 53), (38, 54), (1, 1), (2, 3)])
def test_frame_to_bgr_equals_the_restatement(hw):
    import caffe

    h, w = hw
    y, uv = _planes(h, w, 5, w + 11, 2 * ((w + 1) // 2) + 6)
    for m in NR.MATRICES:
        for r in NR.RANGES:
            f = caffe.Frame.nv12(y, uv, matrix=m, range=r)
            assert (f.height, f.width, f.shape) == (h, w, (h, w, 3))
            assert f.pitches == [w + 11, 2 * ((w + 1) // 2) + 6]
            got = f.to_bgr()
            assert got.dtype == np.uint8 and np.array_equal(got, NR.to_bgr(y, uv, m, r, h, w))
    # a pitched BGR frame is its own pixels
    buf = np.full((h, 3 * w + 5), 0xFF, np.uint8)
    view = np.lib.stride_tricks.as_strided(buf, (h, w, 3), (3 * w + 5, 3, 1))
    view[...] = np.random.RandomState(6).randint(0, 256, (h, w, 3))
    f = caffe.Frame.bgr(view)
    assert f.pitches[0] == 3 * w + 5 and f.shape == (h, w, 3) and np.array_equal(f.to_bgr(), view)


def test_frame_construction_refusals_need_no_device():
    import caffe

    y, uv = _planes(37, 53, 7)
    caffe.Frame.nv12(y, uv)
    for bad_uv in (uv[:, :-1], uv[:-1], uv[:, :, :1], np.zeros((19, 27), np.uint8)):
        with pytest.raises(ValueError, match="uv must have shape"):
            caffe.Frame.nv12(y, bad_uv)
    with pytest.raises(ValueError, match="y must be"):
        caffe.Frame.nv12(np.zeros((37, 53, 1), np.uint8), uv)
    with pytest.raises(ValueError, match="uint8"):
        caffe.Frame.nv12(y.astype(np.int32), uv)
    # inner strides: every other column of a wider plane, a transposed plane, Cb / Cr planes of their own
    wide = np.zeros((37, 106), np.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        caffe.Frame.nv12(wide[:, ::2], uv)
    with pytest.raises(ValueError, match="contiguous"):
        caffe.Frame.nv12(np.zeros((53, 37), np.uint8).T, uv)
    planar = np.zeros((2, 19, 27), np.uint8)
    with pytest.raises(ValueError, match="contiguous"):
        caffe.Frame.nv12(y, planar.transpose(1, 2, 0))
    with pytest.raises(ValueError, match="contiguous"):
        caffe.Frame.bgr(np.zeros((37, 53, 4), np.uint8)[:, :, :3])
    with pytest.raises(ValueError, match="shape"):
        caffe.Frame.bgr(np.zeros((37, 53, 4), np.uint8))
    with pytest.raises(ValueError, match="matrix"):
        caffe.Frame.nv12(y, uv, matrix="bt2020")
    with pytest.raises(ValueError, match="range"):
        caffe.Frame.nv12(y, uv, range="video")
    with pytest.raises(ValueError, match="host frames only"):
        caffe.Frame.nv12_device(4096, 8192, 37, 53, 64, 64).to_bgr()

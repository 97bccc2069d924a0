"""An independent restatement of the NV12 conversion rule of include/deepcut_hip.h (dc_frame), in plain integer numpy.  No import from
the product: the tests hold `caffe.Frame.to_bgr` and the device readers to THIS.

Siting: the pixel at (x, y) uses chroma sample (x >> 1, y >> 1), no interpolation.  c = Y - y0, d = Cb - 128, e = Cr - 128;
limited range: y0 = 16, sy = 255/219, sc = 255/224; full range: y0 = 0, sy = sc = 1; Kg = 1 - Kr - Kb.  Coefficients in double,
rounded to nearest; then int32 with an arithmetic shift:
    R = clip8((ky c + rv e + 32768) >> 16), G = clip8((ky c + gu d + gv e + 32768) >> 16), B = clip8((ky c + bu d + 32768) >> 16)."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRICES, RANGES = ("bt601", "bt709"), ("limited", "full")


def scales(range_):
    """-> (y0, sy, sc)"""
    if range_ == "limited":
        return 16, 255.0 / 219.0, 255.0 / 224.0
    assert range_ == "full"
    return 0, 1.0, 1.0


def coefficients(matrix, range_):
    """-> (ky, rv, bu, gu, gv) as Python ints."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    _, sy, sc = scales(range_)
    vals = (sy, 2.0 * (1.0 - kr) * sc, 2.0 * (1.0 - kb) * sc, (-2.0 * kb * (1.0 - kb) / kg) * sc, (-2.0 * kr * (1.0 - kr) / kg) * sc)
    return tuple(int(np.rint(65536.0 * v)) for v in vals)


def convert(Y, Cb, Cr, matrix, range_):
    """Integer arrays of one shape -> (R, G, B) int32 arrays, by the rule."""
    ky, rv, bu, gu, gv = coefficients(matrix, range_)
    y0 = scales(range_)[0]
    c = np.asarray(Y, np.int32) - np.int32(y0)
    d = np.asarray(Cb, np.int32) - np.int32(128)
    e = np.asarray(Cr, np.int32) - np.int32(128)
    r = np.right_shift(ky * c + rv * e + 32768, 16)  # numpy's >> on signed integers is arithmetic
    g = np.right_shift(ky * c + gu * d + gv * e + 32768, 16)
    b = np.right_shift(ky * c + bu * d + 32768, 16)
    return tuple(np.clip(v, 0, 255).astype(np.int32) for v in (r, g, b))


def real_valued(Y, Cb, Cr, matrix, range_):
    """The float64 matrix of the standard, rounded half-up and clipped -> (R, G, B) int32 arrays."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = scales(range_)
    c = sy * (np.asarray(Y, np.float64) - y0)
    d = sc * (np.asarray(Cb, np.float64) - 128.0)
    e = sc * (np.asarray(Cr, np.float64) - 128.0)
    r = c + 2.0 * (1.0 - kr) * e
    b = c + 2.0 * (1.0 - kb) * d
    g = c - (2.0 * kb * (1.0 - kb) / kg) * d - (2.0 * kr * (1.0 - kr) / kg) * e
    return tuple(np.clip(np.floor(v + 0.5), 0, 255).astype(np.int32) for v in (r, g, b))


def to_bgr(y, uv, matrix, range_, H, W):
    """y: [>= H, >= W] uint8; uv: [>= (H+1)//2, >= (W+1)//2, 2] uint8 (Cb, Cr) -> uint8 [H, W, 3] B, G, R."""
    rows, cols = np.arange(H) // 2, np.arange(W) // 2
    Y = np.asarray(y)[:H, :W]
    cb = np.asarray(uv)[rows][:, cols, 0]
    cr = np.asarray(uv)[rows][:, cols, 1]
    r, g, b = convert(Y, cb, cr, matrix, range_)
    return np.stack([b, g, r], axis=2).astype(np.uint8)

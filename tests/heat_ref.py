"""An independent restatement of the score-map overlay's rule of include/deepcut_hip.h (dc_draw_heatmap), in plain integer numpy plus
float32 for the one quantisation.  No import from the product: the tests hold `caffe.draw_heatmap` to THIS, byte for byte.

PARITY UNPINNED BY THE REFERENCE: its demo draws 14 numpy circles and never shows a map; the rule is this project's own.

q = rint(clamp01(float32 s) * 4096) (NaN -> 0); per axis t = rint(256 * (((x + 0.5 - origin) * scale - 4) / 8)) in double, one numpy
operation per step, clamped to [0, 256 (cells - 1)], i0 = t >> 8, f = t & 255, i1 = min(i0 + 1, cells - 1); NV12 chroma tables at the
block centres 2 b + 1; v = (top (256 - fy) + bot fy + 32768) >> 16 of top / bot = q.0 (256 - fx) + q.1 fx; vmin = rint(4096 min_score);
A(v) = alpha or (alpha v + 2048) >> 12; blend (c A + dst (256 - A) + 128) >> 8 where v >= vmin and A > 0.  "max": the maximum of the
drawn channels' v, colour lut[min(255, v >> 4)]; "joints": the list in order with palette[k % n]."""
import numpy as np

import draw_ref as DR

DEFAULT_STYLE = dict(joints=None, mode="max", alpha=128, alpha_mode="score", min_score=0.0, lut=None, palette=((255, 0, 0),))


def quantise(s):
    """Any float array -> int32 q in [0, 4096], by float32 arithmetic."""
    s = np.asarray(s, np.float32)
    s = np.where(np.isnan(s), np.float32(0), s)
    s = np.minimum(np.maximum(s, np.float32(0)), np.float32(1))
    return np.rint(s * np.float32(4096.0)).astype(np.int32)


def table(count, first, step, origin, scale, cells):
    """-> int64 t [count]: sample point i at pixel coordinate first + step * i."""
    c = np.float64(first) + np.float64(step) * np.arange(count, dtype=np.float64)
    d = c - np.float64(origin)
    m = d * np.float64(scale)
    n = m - np.float64(4.0)
    u = n / np.float64(8.0)
    t = np.rint(np.float64(256.0) * u).astype(np.int64)
    return np.clip(t, 0, 256 * (cells - 1))


def luma_tables(h, w, hm, wm, scale, origin):
    return table(w, 0.5, 1.0, origin[0], scale, wm), table(h, 0.5, 1.0, origin[1], scale, hm)


def chroma_tables(h, w, hm, wm, scale, origin):
    return table((w + 1) // 2, 1.0, 2.0, origin[0], scale, wm), table((h + 1) // 2, 1.0, 2.0, origin[1], scale, hm)


def interpolate(q, tx, ty):
    """q int32 [Hm, Wm], tables -> v int32 [len(ty), len(tx)]."""
    hm, wm = q.shape
    i0, fx = (tx >> 8).astype(np.int64), (tx & 255).astype(np.int32)[None, :]
    j0, fy = (ty >> 8).astype(np.int64), (ty & 255).astype(np.int32)[:, None]
    i1, j1 = np.minimum(i0 + 1, wm - 1), np.minimum(j0 + 1, hm - 1)
    q = q.astype(np.int32)
    top = q[j0][:, i0] * (256 - fx) + q[j0][:, i1] * fx
    bot = q[j1][:, i0] * (256 - fx) + q[j1][:, i1] * fx
    return (top * (256 - fy) + bot * fy + 32768) >> 16


def _alpha(v, alpha, alpha_mode):
    return np.full_like(v, alpha) if alpha_mode == "const" else (alpha * v + 2048) >> 12


def _blend(dst, c, a, mask):
    """dst uint8 array blended in place with colour value(s) c (int or int array) at alpha a where mask."""
    out = (c * a + dst.astype(np.int32) * (256 - a) + 128) >> 8
    dst[mask] = out[mask].astype(np.uint8)


def layers(scores, tx, ty, style):
    """One image's scores [C, Hm, Wm] on the sample grid -> the blends in order: [(mask, alpha int32 [h, w], colour index int32 [h, w] or
    int)]; "max": one layer whose colour indexes the lut, "joints": one per listed channel whose colour is the list place k."""
    st = dict(DEFAULT_STYLE, **style)
    joints = list(range(scores.shape[0])) if st["joints"] is None else list(st["joints"])
    vmin = int(np.rint(4096.0 * st["min_score"]))
    vs = [interpolate(quantise(scores[c]), tx, ty) for c in joints]
    out = []
    if st["mode"] == "max":
        v = np.maximum.reduce(vs)
        a = _alpha(v, st["alpha"], st["alpha_mode"])
        out.append(((v >= vmin) & (a > 0), a, np.minimum(255, v >> 4)))
    else:
        for k, v in enumerate(vs):
            a = _alpha(v, st["alpha"], st["alpha_mode"])
            out.append(((v >= vmin) & (a > 0), a, k))
    return out


def draw_bgr(img, scores, scale, origin=(0.0, 0.0), **style):
    """img uint8 [H, W, 3] B, G, R, blended in place (a strided view is fine: only the pixels are written)."""
    st = dict(DEFAULT_STYLE, **style)
    h, w = img.shape[:2]
    tx, ty = luma_tables(h, w, scores.shape[1], scores.shape[2], scale, origin)
    for mask, a, idx in layers(scores, tx, ty, style):
        rgb = _colour_of(st, idx)
        for ch in range(3):  # B, G, R <- rgb[2], rgb[1], rgb[0]
            plane = img[:, :, ch]
            _blend(plane, rgb[2 - ch], a, mask)


def draw_nv12(y, uv, scores, scale, origin=(0.0, 0.0), matrix="bt601", range_="limited", **style):
    """y uint8 [H, W], uv uint8 [(H+1)//2, (W+1)//2, 2], blended in place."""
    st = dict(DEFAULT_STYLE, **style)
    h, w = y.shape
    hm, wm = scores.shape[1:]
    tx, ty = luma_tables(h, w, hm, wm, scale, origin)
    for mask, a, idx in layers(scores, tx, ty, style):
        Y, _, _ = DR.forward(*_colour_of(st, idx), matrix, range_)
        _blend(y, Y, a, mask)
    cx, cy = chroma_tables(h, w, hm, wm, scale, origin)
    for mask, a, idx in layers(scores, cx, cy, style):
        _, Cb, Cr = DR.forward(*_colour_of(st, idx), matrix, range_)
        _blend(uv[:, :, 0], Cb, a, mask)
        _blend(uv[:, :, 1], Cr, a, mask)


def _colour_of(st, idx):
    """-> (R, G, B), each an int or an int32 array of the layer's shape."""
    if st["mode"] == "max":
        lut = np.asarray(st["lut"], np.int32).reshape(256, 3)
        return lut[idx, 0], lut[idx, 1], lut[idx, 2]
    pal = np.asarray(st["palette"], np.int32).reshape(-1, 3)
    r, g, b = pal[idx % len(pal)]
    return int(r), int(g), int(b)

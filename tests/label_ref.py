"""An independent restatement of the label rule of include/deepcut_hip.h (dc_label_people), in plain Python integers and integer numpy,
written from the rule and not from the C++.  The tests hold `caffe.label_people` and the device routes to THIS, byte for byte.  Of the
product it takes only the font table, through `caffe.LABEL_FONT`, so that it reads the table the kernels read.

PARITY UNPINNED BY THE REFERENCE: its demo draws with matplotlib and labels nothing; the rule is this project's own.

Text: the key is ids[p] (p without ids); key < 0 makes no text; else prefix + decimal key.  A non-empty `texts` entry replaces it.
Held joints as in drawing; a person without one gets no label.  n characters at scale s: tw = s (6 n - 1), th = 7 s, pw = tw + 2 s,
ph = th + 2 s.  Anchor joint held: X = (qx >> 4) - (pw >> 1), Yb = qy >> 4; else the upper left of the held joints' bounding box.
Y = Yb - gap - ph; X, Y clamped to [0, max(0, W - pw)] and [0, max(0, H - ph)].  Layers: the plate rectangle, then the text (u = px - X
- s, v = py - Y - s, k = u / s, glyph i = k / 6, column c = k % 6, row r = v / s, covered when c < 5 and bit 4 - c of the row is
set); a layer whose alpha is 0 is not made.  Blend as in drawing; the NV12 chroma sample once per LAYER."""
import numpy as np

import draw_ref

DEFAULT_STYLE = dict(scale=2, gap=2, anchor=None, prefix="", alpha_text=256, alpha_plate=160, min_score=0.0, color="plate",
                     palette=((255, 0, 0),), text_color=(255, 255, 255), plate_color=(0, 0, 0))


def font():
    import caffe
    return caffe.LABEL_FONT


def make_text(key, prefix="", text=None):
    """-> the text of a person, upper-cased, or None when there is none."""
    if text:
        return text.upper()
    if key < 0:
        return None
    return prefix.upper() + str(int(key))


def held_joints(pose, min_score):
    """pose [J, 3] -> a list per joint: the snapped (qx, qy), or None when the joint is not held."""
    out = []
    for x, y, s in np.asarray(pose, np.float64):
        ok = bool(np.isfinite(x) and np.isfinite(y) and np.isfinite(s) and s > min_score)
        out.append((draw_ref.snap(x), draw_ref.snap(y)) if ok else None)
    return out


def place(held, n, H, W, scale=2, gap=2, anchor=None):
    """-> (X, Y, pw, ph) of a label of n characters, or None without a held joint.  Python's >> and // on ints are arithmetic / floor."""
    pts = [q for q in held if q is not None]
    if not pts:
        return None
    s = int(scale)
    pw, ph = s * (6 * n - 1) + 2 * s, 7 * s + 2 * s
    if anchor is not None and anchor >= 0 and held[anchor] is not None:
        X, Yb = (held[anchor][0] >> 4) - (pw >> 1), held[anchor][1] >> 4
    else:
        X, Yb = min(q[0] for q in pts) >> 4, min(q[1] for q in pts) >> 4
    Y = Yb - int(gap) - ph
    X = min(max(X, 0), max(0, W - pw))
    Y = min(max(Y, 0), max(0, H - ph))
    return X, Y, pw, ph


def labels(people, H, W, n_people=None, ids=None, texts=None, **style):
    """The ordered label list of ONE image: dicts X, Y, pw, ph, s, text, plate_rgb, text_rgb, alpha_text, alpha_plate.  people [P, J, 3]."""
    st = dict(DEFAULT_STYLE, **style)
    people = np.asarray(people, np.float64)
    n = people.shape[0] if n_people is None else int(n_people)
    pal = [tuple(int(v) for v in c) for c in st["palette"]]
    out = []
    if st["alpha_text"] == 0 and st["alpha_plate"] == 0:
        return out
    for p in range(n):
        key = p if ids is None else int(np.asarray(ids).reshape(-1)[p])
        text = make_text(key, st["prefix"], None if texts is None or p >= len(texts) else texts[p])
        if text is None:
            continue
        g = place(held_joints(people[p], st["min_score"]), len(text), H, W, st["scale"], st["gap"], st["anchor"])
        if g is None:
            continue
        person = pal[key % len(pal)] if key >= 0 else pal[0]
        plate, ink = (person, tuple(st["text_color"])) if st["color"] == "plate" else (tuple(st["plate_color"]), person)
        out.append(dict(X=g[0], Y=g[1], pw=g[2], ph=g[3], s=int(st["scale"]), text=text, plate_rgb=tuple(int(v) for v in plate),
                        text_rgb=tuple(int(v) for v in ink), alpha_text=int(st["alpha_text"]), alpha_plate=int(st["alpha_plate"])))
    return out


def layers(lab, H, W):
    """-> [(bool [H, W] mask, rgb, alpha)] of a label's made layers, in order: the plate, then the text."""
    out = []
    px, py = np.arange(W)[None, :], np.arange(H)[:, None]
    X, Y, s = lab["X"], lab["Y"], lab["s"]
    if lab["alpha_plate"] > 0:
        out.append(((px >= X) & (px < X + lab["pw"]) & (py >= Y) & (py < Y + lab["ph"]), lab["plate_rgb"], lab["alpha_plate"]))
    if lab["alpha_text"] > 0:
        f = font()
        n = len(lab["text"])
        tw, th = s * (6 * n - 1), 7 * s
        mask = np.zeros((H, W), bool)
        for y in range(max(0, Y + s), min(H, Y + s + th)):
            for x in range(max(0, X + s), min(W, X + s + tw)):
                u, v = x - X - s, y - Y - s
                k = u // s
                i, c, r = k // 6, k % 6, v // s
                mask[y, x] = c < 5 and bool(f[lab["text"][i]][r] >> (4 - c) & 1)
        out.append((mask, lab["text_rgb"], lab["alpha_text"]))
    return out


def label_bgr(img, labs):
    """img: uint8 [H, W, 3] B, G, R (a view of a pitched buffer is fine) — written in place."""
    H, W = img.shape[:2]
    for lab in labs:
        for m, rgb, A in layers(lab, H, W):
            for ch, c in enumerate(rgb[::-1]):
                plane = img[:, :, ch]
                plane[m] = draw_ref._blend(c, plane[m], A).astype(np.uint8)


def label_nv12(y, uv, labs, matrix, range_):
    """y: uint8 [H, W], uv: uint8 [(H+1)//2, (W+1)//2, 2] (views of pitched buffers are fine) — written in place."""
    H, W = y.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2

    def blocks(mask):
        full = np.zeros((2 * H2, 2 * W2), np.int32)
        full[:H, :W] = mask
        return full.reshape(H2, 2, W2, 2).sum(axis=(1, 3))

    n = blocks(np.ones((H, W), bool))
    for lab in labs:
        for m, rgb, A in layers(lab, H, W):
            Y, Cb, Cr = (int(v) for v in draw_ref.forward(*rgb, matrix, range_))
            y[m] = draw_ref._blend(Y, y[m], A).astype(np.uint8)
            k = blocks(m)
            hit = k > 0
            ac = (A * k[hit] + n[hit] // 2) // n[hit]
            for ch, c in ((0, Cb), (1, Cr)):
                plane = uv[:, :, ch]
                plane[hit] = draw_ref._blend(c, plane[hit], ac).astype(np.uint8)

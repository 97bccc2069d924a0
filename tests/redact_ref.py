"""An independent restatement of the redaction rule of include/deepcut_hip.h (dc_redact_people), in plain integer numpy.  No import from
the product: the tests hold `caffe.redact_people` to THIS, byte for byte.

PARITY UNPINNED BY THE REFERENCE, which has nothing of the kind; the rule is this project's own.

A joint is held when x, y and score are finite and score > min_score; held coordinates are clamped to +-32768 px and snapped to 1/16 px
(rint, ties to even).  Person p takes part when p < n_people and select[p] != 0.  clamp(v, lo, hi) = min(max(v, lo), hi) in float64.
The head disc (both joints of the pair held): centre ((ax + bx) >> 1, (ay + by) >> 1), radius clamp(rint(head_scale * sqrt(L)),
rint(16 min_radius), rint(16 max_radius)), L = d.d.  The body primitives: held limbs as capsules, held joints as discs, radius
clamp(rint(body_scale * s16), rint(16 min_radius), 1024), s16 the larger side of the held joints' bounding box.  "head": the disc; "body":
the disc and the body primitives; "head_or_body": the disc when the pair is held, else the body primitives.  A primitive of radius 0 is
not made; `redacted` is 1 where one was made.  A pixel is covered when its centre (16 px + 8, 16 py + 8) passes the drawing rule's int64
disc / capsule test; a B x B block (grid at (0, 0)) with a covered in-frame pixel is selected.  MOSAIC: every channel of the block's
in-frame pixels becomes (sum + n // 2) // n; NV12 chroma samples (cx, cy) with pixel (2 cx, 2 cy) in the block become (sum + m // 2) // m.
FILL: they become the fill colour (NV12: through the forward colour rule).  Nothing else changes."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
DEFAULT_STYLE = dict(region="head", head=(12, 13), edges=(), head_scale=0.75, body_scale=0.06, min_radius=4.0, max_radius=256.0, min_score=0.0,
                     effect="mosaic", block=8, fill=(0, 0, 0))
BODY_CAP = 1024  # 1/16 px


def forward_colour(rgb, matrix, range_):
    """(R, G, B) -> (Y, Cb, Cr) Python ints by the forward colour rule stated under dc_draw_people."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = (16, 255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (0, 1.0, 1.0)
    r = lambda v: int(np.rint(v))  # noqa: E731
    cy = [r(65536.0 * k / sy) for k in (kr, kg, kb)]
    cb = [r(65536.0 * k / (2.0 * (1.0 - kb)) / sc) for k in (-kr, -kg, 1.0 - kb)]
    cr = [r(65536.0 * k / (2.0 * (1.0 - kr)) / sc) for k in (1.0 - kr, -kg, -kb)]
    mix = lambda c: (c[0] * int(rgb[0]) + c[1] * int(rgb[1]) + c[2] * int(rgb[2]) + 32768) >> 16  # noqa: E731  (Python's >> is arithmetic)
    clip = lambda v: min(255, max(0, v))  # noqa: E731
    return clip(y0 + mix(cy)), clip(128 + mix(cb)), clip(128 + mix(cr))


def snap(v):
    return int(np.rint(16.0 * min(32768.0, max(-32768.0, float(v)))))


def _clamp(v, lo, hi):
    return int(min(max(float(v), float(lo)), float(hi)))


def primitives(people, n_people=None, select=None, **style):
    """The region primitives of ONE image -> (list of dicts a, b, r16, capsule; redacted int32 [P]).  people [P, J, 3]."""
    st = dict(DEFAULT_STYLE, **style)
    people = np.asarray(people, np.float64)
    P, J = people.shape[:2]
    n = P if n_people is None else int(n_people)
    r_lo, r_hi = np.rint(16.0 * st["min_radius"]), np.rint(16.0 * st["max_radius"])
    ha, hb = st["head"]
    out, redacted = [], np.zeros(P, np.int32)
    for p in range(n):
        if select is not None and not int(np.asarray(select)[p]):
            continue
        held = [bool(np.isfinite(people[p, j]).all() and people[p, j, 2] > st["min_score"]) for j in range(J)]
        q = [(snap(people[p, j, 0]), snap(people[p, j, 1])) if held[j] else None for j in range(J)]
        mine = []
        head = held[ha] and held[hb]
        if head:
            dx, dy = q[hb][0] - q[ha][0], q[hb][1] - q[ha][1]
            L = dx * dx + dy * dy  # a Python int
            r16 = _clamp(np.rint(np.float64(st["head_scale"]) * np.sqrt(np.float64(L))), r_lo, r_hi)
            c = ((q[ha][0] + q[hb][0]) >> 1, (q[ha][1] + q[hb][1]) >> 1)
            mine.append(dict(a=c, b=c, r16=r16, capsule=False))
        if st["region"] == "body" or (st["region"] == "head_or_body" and not head):
            pts = [v for v in q if v is not None]
            s16 = max(max(x for x, _ in pts) - min(x for x, _ in pts), max(y for _, y in pts) - min(y for _, y in pts)) if pts else 0
            rb16 = _clamp(np.rint(np.float64(st["body_scale"]) * np.float64(s16)), r_lo, BODY_CAP)
            for a, c in st["edges"]:
                if held[a] and held[c]:
                    mine.append(dict(a=q[a], b=q[c], r16=rb16, capsule=True))
            for j in range(J):
                if held[j]:
                    mine.append(dict(a=q[j], b=q[j], r16=rb16, capsule=False))
        mine = [m for m in mine if m["r16"] >= 1]
        redacted[p] = 1 if mine else 0
        out += mine
    return out, redacted


def coverage(H, W, prim):
    """-> bool [H, W]: the pixels whose centre the primitive covers, in int64 (the drawing rule's test, its guard included)."""
    px = (16 * np.arange(W, dtype=np.int64) + 8)[None, :]
    py = (16 * np.arange(H, dtype=np.int64) + 8)[:, None]
    a, b = prim["a"], prim["b"]
    r2 = np.int64(prim["r16"]) * np.int64(prim["r16"])
    wx, wy = px - np.int64(a[0]), py - np.int64(a[1])
    inside = wx * wx + wy * wy <= r2
    if not prim["capsule"]:
        return inside
    vx, vy = px - np.int64(b[0]), py - np.int64(b[1])
    inside = inside | (vx * vx + vy * vy <= r2)
    dx, dy = np.int64(b[0]) - np.int64(a[0]), np.int64(b[1]) - np.int64(a[1])
    L = dx * dx + dy * dy
    dot = wx * dx + wy * dy
    cross = wx * dy - wy * dx
    small = np.abs(cross) < (np.int64(1) << 31)
    c = np.where(small, cross, 0)  # the square is formed only below 2^62
    return inside | ((dot > 0) & (dot < L) & small & (c * c <= r2 * L))


def selected_blocks(H, W, prims, block):
    """-> the set of (by, bx) block coordinates that hold a covered in-frame pixel."""
    covered = np.zeros((H, W), bool)
    for p in prims:
        covered |= coverage(H, W, p)
    ys, xs = np.nonzero(covered)
    return set(zip((ys // block).tolist(), (xs // block).tolist()))


def _mean(values):
    """(sum + n // 2) // n over a uint8 array, in Python ints."""
    n = int(values.size)
    return (sum(int(v) for v in values.ravel()) + n // 2) // n


def redact_bgr(img, prims, effect="mosaic", block=8, fill=(0, 0, 0)):
    """img: uint8 [H, W, 3] B, G, R (a view of a pitched buffer is fine) — redacted in place.  -> the selected blocks."""
    H, W = img.shape[:2]
    blocks = selected_blocks(H, W, prims, block)
    for by, bx in sorted(blocks):
        v = img[by * block:(by + 1) * block, bx * block:(bx + 1) * block]  # clipped to the frame by the slice
        for ch in range(3):
            v[:, :, ch] = _mean(v[:, :, ch]) if effect == "mosaic" else int(fill[2 - ch])
    return blocks


def redact_nv12(y, uv, prims, matrix, range_, effect="mosaic", block=8, fill=(0, 0, 0)):
    """y: uint8 [H, W], uv: uint8 [(H+1)//2, (W+1)//2, 2] (views of pitched buffers are fine) — redacted in place.  -> the blocks."""
    H, W = y.shape
    blocks = selected_blocks(H, W, prims, block)
    Y, Cb, Cr = forward_colour(fill, matrix, range_)
    half = block // 2
    for by, bx in sorted(blocks):
        v = y[by * block:(by + 1) * block, bx * block:(bx + 1) * block]
        v[...] = _mean(v) if effect == "mosaic" else Y
        # the samples (cx, cy) with pixel (2 cx, 2 cy) in the block: the block starts at an even pixel, so cx from bx * B / 2 on, as far
        # as the chroma plane goes
        c = uv[by * half:(by + 1) * half, bx * half:(bx + 1) * half]
        for ch, f in ((0, Cb), (1, Cr)):
            c[:, :, ch] = _mean(c[:, :, ch]) if effect == "mosaic" else f
    return blocks

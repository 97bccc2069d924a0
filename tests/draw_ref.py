"""An independent restatement of the drawing rule of include/deepcut_hip.h (dc_draw_people), in plain integer numpy.  No import from
the product: the tests hold `caffe.draw_people` to THIS, byte for byte.

PARITY UNPINNED BY THE REFERENCE: the reference draws with matplotlib on the host and states no rule; the rule is this project's own.

A joint is drawn when x, y and score are finite and score > min_score; a limb when both its joints are.  Coordinates are clamped to
+-32768 px and snapped to 1/16 px (rint, ties to even); the centre of pixel (px, py) is (16 px + 8, 16 py + 8).  Coverage in int64 with
w = p - a, v = p - b, d = b - a, L = d.d: disc w.w <= r^2; capsule w.w <= r^2 or v.v <= r^2 or (0 < w.d < L and |cross| < 2^31 and
cross^2 <= r^2 L).  People in index order, of a person the limbs in edge order and then the joints; blend (c A + dst (256 - A) + 128) >> 8.
NV12: luma per pixel, the chroma sample of a 2x2 block once per primitive with Ac = (A k + n / 2) / n (k covered of n in-frame pixels)."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
DEFAULT_STYLE = dict(edges=(), joint_radius=4.0, limb_radius=2.0, alpha=256, alpha_filled=128, min_score=0.0, color="id", palette=((255, 0, 0),),
                     untracked=(128, 128, 128))


def forward_coefficients(matrix, range_):
    """-> ((yr, yg, yb), (cb...), (cr...), y0) as Python ints."""
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y0, sy, sc = (16, 255.0 / 219.0, 255.0 / 224.0) if range_ == "limited" else (0, 1.0, 1.0)
    r = lambda v: int(np.rint(v))  # noqa: E731
    return (tuple(r(65536.0 * k / sy) for k in (kr, kg, kb)), tuple(r(65536.0 * k / (2.0 * (1.0 - kb)) / sc) for k in (-kr, -kg, 1.0 - kb)),
            tuple(r(65536.0 * k / (2.0 * (1.0 - kr)) / sc) for k in (1.0 - kr, -kg, -kb)), y0)


def forward(R, G, B, matrix, range_):
    """Integer arrays (or ints) of one shape -> (Y, Cb, Cr) int32 arrays, by the forward rule."""
    cy, cb, cr, y0 = forward_coefficients(matrix, range_)
    R, G, B = (np.asarray(v, np.int32) for v in (R, G, B))
    mix = lambda c: np.right_shift(c[0] * R + c[1] * G + c[2] * B + 32768, 16)  # noqa: E731  (>> on signed integers is arithmetic)
    return tuple(np.clip(v, 0, 255).astype(np.int32) for v in (y0 + mix(cy), 128 + mix(cb), 128 + mix(cr)))


def snap(v):
    return int(np.rint(16.0 * min(32768.0, max(-32768.0, float(v)))))


def coverage(H, W, a, b, r16, capsule):
    """-> (bool [H, W] mask of the covered pixels, the number of pixels that took the |cross| >= 2^31 guard)."""
    px = (16 * np.arange(W, dtype=np.int64) + 8)[None, :]
    py = (16 * np.arange(H, dtype=np.int64) + 8)[:, None]
    r2 = np.int64(r16) * np.int64(r16)
    wx, wy = px - np.int64(a[0]), py - np.int64(a[1])
    inside = wx * wx + wy * wy <= r2
    if not capsule:
        return inside, 0
    vx, vy = px - np.int64(b[0]), py - np.int64(b[1])
    inside = inside | (vx * vx + vy * vy <= r2)
    dx, dy = np.int64(b[0]) - np.int64(a[0]), np.int64(b[1]) - np.int64(a[1])
    L = dx * dx + dy * dy
    dot = wx * dx + wy * dy
    between = (dot > 0) & (dot < L)
    cross = wx * dy - wy * dx
    small = np.abs(cross) < (np.int64(1) << 31)
    c = np.where(small, cross, 0)  # the square is formed only below 2^62
    body = between & small & (c * c <= r2 * L)
    return inside | body, int((between & ~small).sum())


def coverage_exact(H, W, a, b, r16, capsule):
    """The same set by exact Python-integer arithmetic, without the guard."""
    px = (16 * np.arange(W) + 8).astype(object)[None, :]
    py = (16 * np.arange(H) + 8).astype(object)[:, None]
    r2 = int(r16) ** 2
    wx, wy = px - int(a[0]), py - int(a[1])
    inside = (wx * wx + wy * wy <= r2).astype(bool)
    if not capsule:
        return inside
    vx, vy = px - int(b[0]), py - int(b[1])
    dx, dy = int(b[0]) - int(a[0]), int(b[1]) - int(a[1])
    L = dx * dx + dy * dy
    dot = wx * dx + wy * dy
    cross = wx * dy - wy * dx
    body = (dot > 0).astype(bool) & (dot < L).astype(bool) & (cross * cross <= r2 * L).astype(bool)
    return inside | (vx * vx + vy * vy <= r2).astype(bool) | body


def primitives(people, n_people=None, cand=None, ids=None, **style):
    """The ordered primitive list of ONE image: dicts a, b (fixed point), r16, capsule, alpha, rgb.  people [P, J, 3]."""
    st = dict(DEFAULT_STYLE, **style)
    people = np.asarray(people, np.float64)
    n = people.shape[0] if n_people is None else int(n_people)
    J = people.shape[1]
    pal = [tuple(int(v) for v in c) for c in st["palette"]]
    rj, rl = int(np.rint(16.0 * st["joint_radius"])), int(np.rint(16.0 * st["limb_radius"]))
    out = []
    for p in range(n):
        drawn = [bool(np.isfinite(people[p, j]).all() and people[p, j, 2] > st["min_score"]) for j in range(J)]
        q = [(snap(people[p, j, 0]), snap(people[p, j, 1])) if drawn[j] else None for j in range(J)]
        filled = [cand is not None and int(np.asarray(cand)[p, j]) <= -2 for j in range(J)]
        if st["color"] == "id":
            key = p if ids is None else int(np.asarray(ids)[p])
            person = tuple(int(v) for v in st["untracked"]) if key < 0 else pal[key % len(pal)]
        for a, c in ([] if rl == 0 else st["edges"]):
            if drawn[a] and drawn[c]:
                out.append(dict(a=q[a], b=q[c], r16=rl, capsule=True, alpha=st["alpha_filled"] if filled[a] or filled[c] else st["alpha"],
                                rgb=person if st["color"] == "id" else pal[c % len(pal)]))
        for j in range(J if rj else 0):
            if drawn[j]:
                out.append(dict(a=q[j], b=q[j], r16=rj, capsule=False, alpha=st["alpha_filled"] if filled[j] else st["alpha"],
                                rgb=person if st["color"] == "id" else pal[j % len(pal)]))
    return out


def _blend(c, dst, A):
    return np.right_shift(np.int32(c) * A + dst.astype(np.int32) * (256 - A) + 128, 8)


def draw_bgr(img, prims, stats=None):
    """img: uint8 [H, W, 3] B, G, R (a view of a pitched buffer is fine) — drawn in place.  stats: a dict that counts "guard"."""
    H, W = img.shape[:2]
    for p in prims:
        m, g = coverage(H, W, p["a"], p["b"], p["r16"], p["capsule"])
        if stats is not None:
            stats["guard"] = stats.get("guard", 0) + g
        for ch, c in enumerate(p["rgb"][::-1]):
            plane = img[:, :, ch]
            plane[m] = _blend(c, plane[m], p["alpha"]).astype(np.uint8)


def draw_nv12(y, uv, prims, matrix, range_, stats=None):
    """y: uint8 [H, W], uv: uint8 [(H+1)//2, (W+1)//2, 2] (views of pitched buffers are fine) — drawn in place."""
    H, W = y.shape
    H2, W2 = (H + 1) // 2, (W + 1) // 2

    def blocks(mask):
        full = np.zeros((2 * H2, 2 * W2), np.int32)
        full[:H, :W] = mask
        return full.reshape(H2, 2, W2, 2).sum(axis=(1, 3))

    n = blocks(np.ones((H, W), bool))
    for p in prims:
        m, g = coverage(H, W, p["a"], p["b"], p["r16"], p["capsule"])
        if stats is not None:
            stats["guard"] = stats.get("guard", 0) + g
        Y, Cb, Cr = (int(v) for v in forward(*p["rgb"], matrix, range_))
        y[m] = _blend(Y, y[m], p["alpha"]).astype(np.uint8)
        k = blocks(m)
        hit = k > 0
        ac = (p["alpha"] * k[hit] + n[hit] // 2) // n[hit]
        for ch, c in ((0, Cb), (1, Cr)):
            plane = uv[:, :, ch]
            plane[hit] = _blend(c, plane[hit], ac).astype(np.uint8)

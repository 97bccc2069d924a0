"""An independent restatement of the appearance rules of include/deepcut_hip.h, in plain integer numpy and plain loops.  No import from
the product: the tests hold `caffe.describe_people` and the tracker's appearance steps to THIS, exactly.

PARITY UNPINNED BY THE REFERENCE, which stops at the maps; both rules are this project's own.

THE DESCRIPTOR (dc_describe_people).  A joint is held when x, y and score are finite and score > min_score; held coordinates are clamped
to +-32768 px and snapped to 1/16 px (rint, ties to even).  The region of person p: a capsule for every edge whose two joints are held,
of radius r16 = clamp(rint(scale * s16), rint(16 min_radius), 1024), s16 the larger side of the bounding box of the person's held joints
in snapped units; a radius of 0 makes no primitive; there are no joint discs.  A pixel (x, y) of the frame belongs to the region when
its centre (16 x + 8, 16 y + 8) passes the drawing rule's int64 capsule test for ANY of the person's capsules; it counts once per person.
Per region pixel three bytes — BGR24: B, G, R; NV12: Y(x, y), Cb and Cr of sample (x >> 1, y >> 1) — and desc[p][c][v >> 4] += 1."""
import numpy as np

BINS = 16
RADIUS_CAP = 1024  # 1/16 px
DEFAULT_STYLE = dict(edges=(), scale=0.04, min_radius=2.0, min_score=0.0)


def snap(v):
    return int(np.rint(16.0 * min(32768.0, max(-32768.0, float(v)))))


def _clamp(v, lo, hi):
    return int(min(max(float(v), float(lo)), float(hi)))


def capsules(pose, **style):
    """The capsules of ONE person -> list of (ax, ay, bx, by, r16).  pose [J, 3]."""
    st = dict(DEFAULT_STYLE, **style)
    pose = np.asarray(pose, np.float64)
    J = pose.shape[0]
    held = [bool(np.isfinite(pose[j]).all() and pose[j, 2] > st["min_score"]) for j in range(J)]
    q = [(snap(pose[j, 0]), snap(pose[j, 1])) if held[j] else None for j in range(J)]
    pts = [v for v in q if v is not None]
    s16 = max(max(x for x, _ in pts) - min(x for x, _ in pts), max(y for _, y in pts) - min(y for _, y in pts)) if pts else 0
    r16 = _clamp(np.rint(np.float64(st["scale"]) * np.float64(s16)), np.rint(16.0 * st["min_radius"]), RADIUS_CAP)
    if r16 < 1:
        return []
    return [q[a] + q[c] + (r16,) for a, c in st["edges"] if held[a] and held[c]]


def covers(cap, px, py):
    """The drawing rule's capsule test for the point (px, py) in 1/16 px, in Python ints (no overflow to guard)."""
    ax, ay, bx, by, r16 = cap
    r2 = r16 * r16
    wx, wy = px - ax, py - ay
    if wx * wx + wy * wy <= r2:
        return True
    vx, vy = px - bx, py - by
    if vx * vx + vy * vy <= r2:
        return True
    dx, dy = bx - ax, by - ay
    L, dot = dx * dx + dy * dy, wx * dx + wy * dy
    if not 0 < dot < L:
        return False
    cross = wx * dy - wy * dx
    return cross * cross <= r2 * L


def region(H, W, caps):
    """-> bool [H, W]: the in-frame pixels whose centre any of the capsules covers (a plain loop over the capsules' grown boxes)."""
    inside = np.zeros((H, W), bool)
    for cap in caps:
        ax, ay, bx, by, r16 = cap
        x0, x1 = max(0, (min(ax, bx) - r16) // 16 - 1), min(W - 1, (max(ax, bx) + r16) // 16 + 1)
        y0, y1 = max(0, (min(ay, by) - r16) // 16 - 1), min(H - 1, (max(ay, by) + r16) // 16 + 1)
        for y in range(y0, y1 + 1):
            for x in range(x0, x1 + 1):
                if not inside[y, x] and covers(cap, 16 * x + 8, 16 * y + 8):
                    inside[y, x] = True
    return inside


def _count(desc, inside, channels):
    ys, xs = np.nonzero(inside)
    for y, x in zip(ys.tolist(), xs.tolist()):
        for c, ch in enumerate(channels):
            desc[c, int(ch(y, x)) >> 4] += 1


def describe_bgr(img, people, n_people=None, **style):
    """img: uint8 [H, W, 3] B, G, R (a view of a pitched buffer is fine), only read.  people [P, J, 3] -> int32 [P, 3, 16]."""
    H, W = img.shape[:2]
    people = np.asarray(people, np.float64)
    desc = np.zeros((people.shape[0], 3, BINS), np.int32)
    for p in range(people.shape[0] if n_people is None else int(n_people)):
        _count(desc[p], region(H, W, capsules(people[p], **style)), [lambda y, x, c=c: img[y, x, c] for c in range(3)])
    return desc


def describe_nv12(y, uv, people, n_people=None, **style):
    """y: uint8 [H, W], uv: uint8 [(H+1)//2, (W+1)//2, 2], only read.  people [P, J, 3] -> int32 [P, 3, 16]: Y, Cb, Cr."""
    H, W = y.shape
    people = np.asarray(people, np.float64)
    desc = np.zeros((people.shape[0], 3, BINS), np.int32)
    chans = [lambda r, c: y[r, c], lambda r, c: uv[r >> 1, c >> 1, 0], lambda r, c: uv[r >> 1, c >> 1, 1]]
    for p in range(people.shape[0] if n_people is None else int(n_people)):
        _count(desc[p], region(H, W, capsules(people[p], **style)), chans)
    return desc


# ---- the tracker's appearance steps (dc_tracker_update_appearance), on top of tests/track_ref.py's Slot ----------------------------------
# THE RULE, all integer.  A descriptor h [3][16] with n = sum_k h[0][k] >= min_pixels is valid; q[c][k] = (4096 h[c][k] + n // 2) // n.
# A(m, q) = 12288 - sum min(m, q).  Model update: m += ((q - m) * alpha256 + 128) >> 8 (Python's >> is arithmetic); the first valid
# observation sets m = q.  Per slot: model / valid per place, a gallery of 64 entries (id, age, model).  0': every occupied entry ages
# by one and is freed beyond max_age.  5': a matched track whose person has a valid descriptor updates its model.  6': the tracks freed
# in this update, place ascending, with hits >= min_hits and a valid model enter the gallery with age 0 — the lowest free entry, else the
# entry of largest age (the lower index among equals).  7': among the born people with a valid descriptor, while a person and an
# occupied entry with A <= reid_max remain, the pair of smallest (A, entry, person) is taken: the track takes the entry's id, its model
# is the entry's updated with q, the entry is freed.  The other born people take next_id + their rank among them, q ascending.
GALLERY = 64
MODEL = 3 * BINS


def appearance_params(min_pixels=1, alpha256=64, reid_max=4096, max_age=300, min_hits=1):
    return dict(min_pixels=int(min_pixels), alpha256=int(alpha256), reid_max=int(reid_max), max_age=int(max_age), min_hits=int(min_hits))


def quantise(h, min_pixels):
    """h int [3, 16] -> the quantised descriptor as a list of 48 Python ints, or None when it is not valid."""
    h = [[int(v) for v in row] for row in np.asarray(h).reshape(3, BINS)]
    n = sum(h[0])
    if n < min_pixels or n < 1:
        return None
    return [(4096 * v + n // 2) // n for row in h for v in row]


def dissimilarity(m, q):
    return 3 * 4096 - sum(min(int(a), int(b)) for a, b in zip(m, q))


def blend(m, q, alpha256):
    return [int(a) + (((int(b) - int(a)) * alpha256 + 128) >> 8) for a, b in zip(m, q)]


class Appearance(object):
    """The appearance state of one slot: every model not valid, the gallery empty."""

    def __init__(self, T):
        self.T = int(T)
        self.reset()

    def reset(self):
        self.model = [None] * self.T                 # per place: 48 ints, or None = not valid
        self.gallery = [None] * GALLERY              # per entry: [id, age, model], or None = free


def update(slot, app, people, n, P, prm, ap, desc=None, associate=None):
    """One image: steps 1-7 of tests/track_ref.py with 0', 5', 6' and 7' -> (ids int64 [P], place int32 [P], reid int32 [P], D).
    associate: steps 4-7 on given distances — track_ref.associate (the default) or assign_ref.associate.  The plain rule runs on the slot;
    what the appearance steps change of it — the ids of the born people, next_id — is then put right: places, poses, hits and misses are
    the plain rule's by definition."""
    import track_ref as TR

    people = np.asarray(people, np.float64)
    T = slot.T
    q = [None] * P
    for k in range(n if desc is not None else 0):
        q[k] = quantise(desc[k], ap["min_pixels"])
    # 0'
    for g, e in enumerate(app.gallery):
        if e is not None:
            e[1] += 1
            if e[1] > ap["max_age"]:
                app.gallery[g] = None
    was_live, was_id, was_hits, next_id = list(slot.live), list(slot.id), list(slot.hits), slot.next_id
    D = TR.distances(slot, people, n, P, prm)
    ids, place = (associate or TR.associate)(slot, D, people, n, P, prm)
    born = [k for k in range(n) if place[k] >= 0 and ids[k] >= next_id]  # ids are never reused: a new one marks a birth
    born_places = set(int(place[k]) for k in born)
    # 5'
    for k in range(n):
        i = int(place[k])
        if i >= 0 and k not in born and q[k] is not None:
            app.model[i] = list(q[k]) if app.model[i] is None else blend(app.model[i], q[k], ap["alpha256"])
    # 6'
    for i in range(T):
        freed = was_live[i] and (not slot.live[i] or i in born_places)
        if not (freed and was_hits[i] >= ap["min_hits"] and app.model[i] is not None):
            continue
        free = [g for g in range(GALLERY) if app.gallery[g] is None]
        g = free[0] if free else max(range(GALLERY), key=lambda e: (app.gallery[e][1], -e))
        app.gallery[g] = [was_id[i], 0, list(app.model[i])]
    # 7'
    reid = np.zeros(P, np.int32)
    taken = {}
    while True:
        open_ = [(dissimilarity(e[2], q[k]), g, k) for g, e in enumerate(app.gallery) if e is not None
                 for k in born if k not in taken and q[k] is not None]
        open_ = [c for c in open_ if c[0] <= ap["reid_max"]]
        if not open_:
            break
        _a, g, k = min(open_)
        taken[k] = app.gallery[g]
        app.gallery[g] = None
    fresh = 0
    for k in born:
        i = int(place[k])
        if k in taken:
            ids[k], reid[k] = taken[k][0], 1
            app.model[i] = blend(taken[k][2], q[k], ap["alpha256"])
        else:
            ids[k] = next_id + fresh
            fresh += 1
            app.model[i] = None if q[k] is None else list(q[k])
        slot.id[i] = int(ids[k])
    slot.next_id = next_id + fresh
    live_ids = [slot.id[i] for i in range(T) if slot.live[i]]
    assert len(live_ids) == len(set(live_ids)), "an id is live twice"
    assert not set(live_ids) & set(e[0] for e in app.gallery if e is not None), "a live id is in the gallery"
    return ids, place, reid, D


def appearance_state(slot, app):
    """What dc_tracker_appearance_state gives: track_model [T, 3, 16], track_valid [T], gallery_ids [64], gallery_age [64], gallery_model."""
    T = slot.T
    tm, tv = np.zeros((T, 3, BINS), np.int32), np.zeros(T, np.int32)
    for i in range(T):
        if slot.live[i] and app.model[i] is not None:
            tm[i], tv[i] = np.array(app.model[i], np.int32).reshape(3, BINS), 1
    gi, ga, gm = np.full(GALLERY, -1, np.int64), np.full(GALLERY, -1, np.int32), np.zeros((GALLERY, 3, BINS), np.int32)
    for g, e in enumerate(app.gallery):
        if e is not None:
            gi[g], ga[g], gm[g] = e[0], e[1], np.array(e[2], np.int32).reshape(3, BINS)
    return tm, tv, gi, ga, gm

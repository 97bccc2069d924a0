"""Crafted `prob` / `loc_pred` maps for the device map readers of csrc/pose.hip (pose_decode_kernel, plain and restricted to a box's own
cells, part_select_kernel, and both on top of fuse_maps_kernel), and their float64 answers.  Test helper, never on the product path.

The maps reach what the maps of a real forward do not: exact ties (the first-maximum rule of the strided scan and of the LDS tree, the
lower-cell rule of the NMS window), maxima on the map's edges, candidate counts on the boundaries of part_select_kernel's sort (0, 1, just
above a power of two, 4096 against 4097: the LDS sort against the spill path), both signs of zero at threshold 0, NaN cells, and boxes
whose valid cells exclude the map's global maximum.

Every score is a multiple of 1/256 in [0, 1] and every `loc_pred` value a multiple of 1/8 in [-1, 1], so each is exact in float16 and in
bfloat16 (8 significant bits are enough for k / 256, k <= 256) and a net of any element type reads the numbers written here.  The only
other values are the zeros case's 2^-20 / 2^-16 (float16 denormals, exact there and in bfloat16), -0.0, and the NaN case's NaN.

NO SECOND RESTATEMENT: the answers are `pose.estimate_pose.pose_from_maps` (pinned to the reference's `_pose_from_mats` by
tests/test_pose.py), `oracle.multiperson.nms_candidates` and `boxfuse_ref.box_poses`.  nms_candidates' plain loops take about a second
for the largest case here (4160 cells, radius 0, 14 joints), so there is no vectorised path beside it."""
import functools

import numpy as np

J = 14
THR = 0.5  # = 128 / 256
PEAK = 200  # / 256: the value of a planted maximum


def _frozen(**kw):
    for v in kw.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return kw


def loc_map(n, h, w, seed=0):
    """[n, 2J, h, w] multiples of 1/8 in [-1, 1]; neighbouring cells, channels and images differ, so a pose decoded from a wrong cell or
    channel has a wrong refinement too."""
    ch, r, c = np.arange(2 * J)[:, None, None], np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    return np.stack([((3 * r + 5 * c + 7 * ch + 11 * (seed + b)) % 17 - 8) / 8.0 for b in range(n)]).astype(np.float32)


def background(h, w, j, below=64):
    """[h, w] multiples of 1/256 in [0, below / 256): the cells nobody planted."""
    r, c = np.arange(h)[:, None], np.arange(w)[None, :]
    return (((5 * r + 3 * c + 7 * j) % below) / 256.0).astype(np.float32)


# ---- first maximum: pose_decode_kernel's strided scan (thread t reads cells t, t + 256, t + 512) and its LDS tree ----------------------
FIRST_HW = (19, 29)  # 551 cells: three trips of the scan, the last one of 39 cells; not a multiple of 256
_LAST = FIRST_HW[0] * FIRST_HW[1] - 1
# per image and joint: (what, the cells at the maximum); None = every cell (a plateau), () = an all-zero map
FIRST_PATTERNS = (
    (("plateau over the whole map", None),
     ("two maxima one thread apart", (300, 301)),
     ("two maxima one trip apart", (37, 293)),
     ("two maxima in trips 0 and 2 of one thread", (20, 532)),
     ("the larger index in the lower LDS half (threads 200 and 10)", (200, 266)),
     ("the maximum at the last cell", (_LAST,)),
     ("the maximum at cell 255", (255,)),
     ("the maximum at cell 256", (256,)),
     ("an all-zero map", ()),
     ("maxima at cells 255 and 256", (255, 256)),
     ("maxima at the first and the last cell", (0, _LAST)),
     ("maxima in all three trips of one thread", (7, 263, 519)),
     ("maxima in threads 127 and 128", (127, 128)),
     ("the larger index in thread 0 (threads 255 and 0)", (255, 512))),
    (("two maxima one trip apart, the last thread", (255, 511)),
     ("the maximum at cell 256", (256,)),
     ("an all-zero map", ()),
     ("the last cell and the same thread's first", (38, _LAST)),
     ("plateau over the whole map", None),
     ("the larger index in the lower LDS half (threads 129 and 1)", (129, 257)),
     ("two maxima one thread apart across a row end", (28, 29)),
     ("the maximum at cell 255", (255,)),
     ("the maximum at the last cell", (_LAST,)),
     ("maxima in trips 1 and 2 of one thread", (290, 546)),
     ("four maxima, every LDS quarter", (70, 130, 200, 250)),
     ("two maxima in trip 1, threads 3 and 131", (256 + 3, 256 + 131)),
     ("maxima at cells 511 and 512", (511, 512)),
     ("the maximum at cell 0", (0,))),
)


@functools.lru_cache(maxsize=None)
def first_max_case():
    """Batch 2, different patterns per image.  -> prob [2, J, 19, 29], loc [2, 2J, 19, 29], maxima[b][j] = the cells at the maximum
    (ascending; all cells for a plateau or an all-zero map), what[b][j]."""
    h, w = FIRST_HW
    prob = np.zeros((2, J, h, w), np.float32)
    maxima, what = [], []
    for b in range(2):
        assert len(FIRST_PATTERNS[b]) == J
        maxima.append([]), what.append([])
        for j, (name, cells) in enumerate(FIRST_PATTERNS[b]):
            flat = prob[b, j].reshape(-1)
            if cells is None:
                flat[:] = PEAK / 256.0
                cells = tuple(range(h * w))
            elif cells == ():
                cells = tuple(range(h * w))
            else:
                flat[:] = background(h, w, j + 3 * b).reshape(-1)
                flat[list(cells)] = PEAK / 256.0
            maxima[b].append(tuple(cells)), what[b].append(name)
    return _frozen(prob=prob, loc=loc_map(2, h, w, 1), maxima=maxima, what=what)


# ---- NMS windows: part_select_kernel's (2r+1)^2 test on the map's edges, with ties and at the threshold -------------------------------
WINDOW_HW = (16, 23)  # 368 cells: the cell loop takes a second trip
WINDOW_RADII = (1, 3)


@functools.lru_cache(maxsize=None)
def window_case(radius):
    """-> prob [1, J, 16, 23], loc, survivors: {joint: the cells that must come out, in output order} for the crafted joints 0-6 (the
    host test holds nms_candidates to it); joints 7-13 are maps of eight levels around the threshold, ties everywhere."""
    h, w = WINDOW_HW
    r = radius
    assert 1 <= r <= 3
    prob = np.stack([background(h, w, j) for j in range(J)])[None].copy()
    put = lambda j, cells, k: [prob[0, j].__setitem__(rc, k / 256.0) for rc in cells]  # noqa: E731
    cell = lambda rc: rc[0] * w + rc[1]  # noqa: E731
    surv = {}
    # 0: equal maxima in all four corners -> all four, by cell
    corners = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    put(0, corners, PEAK)
    surv[0] = [cell(c) for c in corners]
    # 1: a maximum on each edge, two of them equal
    put(1, [(0, 9)], 210), put(1, [(h - 1, 8)], 190), put(1, [(6, 0)], PEAK), put(1, [(5, w - 1)], PEAK)
    surv[1] = [cell((0, 9)), cell((5, w - 1)), cell((6, 0)), cell((h - 1, 8))]
    # 2: equal pairs inside one window (in a row, and on the window's anti-diagonal corner): the lower cell wins, the other is gone
    put(2, [(3, 3), (3, 3 + r), (10, 15), (10 + r, 15 - r)], PEAK)
    surv[2] = [cell((3, 3)), cell((10, 15))]
    # 3: equal pairs exactly radius + 1 apart (row, column, diagonal): both survive
    pairs = [(3, 3), (3, 4 + r), (9, 14), (10 + r, 14), (9, 2), (10 + r, 3 + r)]
    put(3, pairs, PEAK)
    surv[3] = sorted(cell(c) for c in pairs)
    # 4: a score equal to the threshold stays, one 1/256 step below it goes
    put(4, [(4, 4)], 128), put(4, [(4, 12)], 127), put(4, [(11, 6)], 129)
    surv[4] = [cell((11, 6)), cell((4, 4))]
    # 5: a 4 x 4 block of equal scores: its first cell only
    put(5, [(y, x) for y in range(6, 10) for x in range(8, 12)], 180)
    surv[5] = [cell((6, 8))]
    # 6: a plateau over the whole map: cell 0 only
    prob[0, 6] = 160 / 256.0
    surv[6] = [0]
    rs = np.random.RandomState(100 + r)
    prob[0, 7:] = (96 + 16 * rs.randint(0, 8, (J - 7, h, w))) / 256.0
    return _frozen(prob=prob.astype(np.float32), loc=loc_map(1, h, w, 2), survivors=surv)


# ---- counts: radius 0, every cell at or above the threshold is a candidate -------------------------------------------------------------
COUNT_HW = (64, 65)  # 4160 cells
# one joint per count.  0 and 1; 257 (just above a power of two: the zero-key padding of the bitonic sort); 4096 (= kPartLds, the LDS sort)
# against 4097 (the spill path); then their neighbours, every cell, and a few more powers of two + 1
COUNTS = (0, 1, 257, 4096, 4097, 2, 255, 256, 258, 4095, 4160, 1025, 2049, 96)
COUNT_LEVELS = (128, 160, 192, 255)  # four scores for up to 4160 candidates: within a score the order is by cell alone


@functools.lru_cache(maxsize=None)
def counts_case():
    """-> prob [1, J, 64, 65] with exactly COUNTS[j] cells of joint j at or above THR, loc."""
    h, w = COUNT_HW
    assert len(COUNTS) == J
    cells = np.arange(h * w)
    prob = np.zeros((1, J, h, w), np.float32)
    for j, n in enumerate(COUNTS):
        flat = prob[0, j].reshape(-1)
        flat[:] = np.where(cells % 3 == 0, 127, cells % 100) / 256.0  # everything else: one step below the threshold, or lower
        at = np.random.RandomState(200 + j).permutation(h * w)[:n]
        flat[at] = np.asarray(COUNT_LEVELS)[(at * 7 + j) % 4] / 256.0
    return _frozen(prob=prob, loc=loc_map(1, h, w, 3))


# ---- zeros: threshold 0 and both signs of zero -----------------------------------------------------------------------------------------
ZERO_HW = (9, 11)
ZERO_MAX_DET = 40  # 99 candidates per joint at radius 0, 33 or 34 of them positive: six or seven zeros are listed, in cell order whatever their sign


@functools.lru_cache(maxsize=None)
def zeros_case(tiny_exp=-20):
    """+0.0, -0.0, one float16-denormal-sized score 2^tiny_exp and ordinary scores, in a pattern of period 6 whose phase moves with the
    joint.  -> prob [1, J, 9, 11], loc."""
    h, w = ZERO_HW
    cells = np.arange(h * w)
    prob = np.zeros((1, J, h, w), np.float32)
    for j in range(J):
        k = (cells + j) % 6
        flat = prob[0, j].reshape(-1)
        flat[:] = 0.0  # k == 2, and k == 0 of the even joints
        flat[k == 3] = (64 + (cells[k == 3] * 5) % 192) / 256.0
        flat[k == 5] = (1 + (cells[k == 5] * 3) % 60) / 256.0
        flat[(k == 1) | (k == 4)] = -0.0
        if j % 2:
            flat[k == 0] = -0.0
        flat[np.flatnonzero(k == 5)[j % 3]] = np.float32(2.0) ** tiny_exp
    return _frozen(prob=prob, loc=loc_map(1, h, w, 4))


# ---- NaN cells next to maxima: never selected, never suppressing a neighbour -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nan_case():
    """-> prob [1, J, 9, 11] (joints 0-2 crafted, the others eight levels with six NaN cells each), loc."""
    h, w = ZERO_HW
    rs = np.random.RandomState(300)
    prob = ((96 + 16 * rs.randint(0, 8, (1, J, h, w))) / 256.0).astype(np.float32)
    for j in range(3):
        prob[0, j] = background(h, w, j)
    prob[0, 0, 4, 5] = PEAK / 256.0  # a maximum with NaN to its left and above it
    prob[0, 0, 4, 4] = prob[0, 0, 3, 5] = np.nan
    prob[0, 1, 0, 0] = np.nan  # NaN in a corner beside the maximum, and at the last cell
    prob[0, 1, 0, 1] = PEAK / 256.0
    prob[0, 1, h - 1, w - 1] = np.nan
    prob[0, 2, 2, 2] = prob[0, 2, 2, 4] = PEAK / 256.0  # NaN between two equal maxima two cells apart
    prob[0, 2, 2, 3] = np.nan
    for j in range(3, J):
        prob[0, j].reshape(-1)[rs.choice(h * w, 6, replace=False)] = np.nan
    return _frozen(prob=prob, loc=loc_map(1, h, w, 5))


# ---- restricted decode: the box entry's valid cells [0, rows) x [0, cols) of a map over the common canvas ------------------------------
BOX_IMAGE_HW = (170, 240)
BOX_CANVAS = (160, 232)  # map 20 x 29 = 580 cells
# (x0, y0, x1, y1), scale -> valid cells rows x cols:
BOXES = [(0, 0, 232, 100),    # 13 x 29: full width (cols == W), 377 cells
         (3, 5, 153, 146),    # 18 x 19: narrow, 342 cells — the (q / cols) * W + q % cols walk past its first trip
         (50, 60, 55, 66),    # 1 x 1
         (8, 2, 240, 162),    # 20 x 29: rows and cols end at the canvas edge (the whole map)
         (100, 10, 140, 170)]  # at scale 0.5: 10 x 3
BOX_SCALES = [1.0, 1.0, 1.0, 1.0, 0.5]
BOX_REGIONS = [(13, 29), (18, 19), (1, 1), (20, 29), (10, 3)]
OUTSIDE = 255  # / 256: the global maximum of every joint, outside the region
BOX_PATTERNS = ("two maxima next to each other", "two maxima 256 cells of the walk apart", "the maximum at the region's last cell",
                "maxima at the region's first and last cell", "a plateau over the region", "two maxima across a row end of the region")


def _region_cells(pattern, rows, cols):
    """-> the region's cells at its maximum, as walk indices q = row * cols + col."""
    cnt = rows * cols
    if cnt == 1:
        return [0]
    if pattern == 0:
        q = min(cnt // 2, cnt - 2)
        return [q, q + 1]
    if pattern == 1:
        return [cnt // 5, cnt // 5 + 256] if cnt // 5 + 256 < cnt else [cnt // 5, cnt - 1]
    if pattern == 2:
        return [cnt - 1]
    if pattern == 3:
        return [0, cnt - 1]
    if pattern == 4:
        return list(range(cnt))
    row = min(rows // 2, rows - 2) if rows > 1 else 0
    return [row * cols + cols - 1, (row + 1) * cols] if rows > 1 else [cols - 2, cols - 1]


@functools.lru_cache(maxsize=None)
def restricted_case():
    """One map per box over the 20 x 29 canvas map.  Inside box i's region joint j carries BOX_PATTERNS[(i + j) % 6] at PEAK / 256 over a
    background below 64 / 256; every cell outside the region is 255 / 256 (where j + cell is a multiple of 3), PEAK / 256 (a tie with the
    region's maximum that an unrestricted walk would meet first, e.g. in row 0 to the right of a narrow region) or background.
    -> prob [5, J, 20, 29], loc, regions, inside[i][j] = the region's cells (map indices) at its maximum."""
    H, W = BOX_CANVAS[0] // 8, BOX_CANVAS[1] // 8
    n = len(BOXES)
    prob = np.zeros((n, J, H, W), np.float32)
    inside = []
    rr, cc = np.arange(H)[:, None], np.arange(W)[None, :]
    for i, (rows, cols) in enumerate(BOX_REGIONS):
        inside.append([])
        out = (rr >= rows) | (cc >= cols)
        for j in range(J):
            m = background(H, W, i + j)
            k = (rr * W + cc + j) % 3
            m[out & (k == 0)] = OUTSIDE / 256.0
            m[out & (k == 1)] = PEAK / 256.0
            cells = [(q // cols) * W + q % cols for q in _region_cells((i + j) % 6, rows, cols)]
            m.reshape(-1)[cells] = PEAK / 256.0
            prob[i, j] = m
            inside[i].append(cells)
    return _frozen(prob=prob, loc=loc_map(n, H, W, 6), inside=inside)


# ---- the float64 answers ---------------------------------------------------------------------------------------------------------------
def poses(prob, loc, scale):
    """pose_from_maps of every image.  -> float64 [n, 5, J]."""
    from pose.estimate_pose import pose_from_maps

    return np.stack([pose_from_maps(prob[b], loc[b], scale) for b in range(prob.shape[0])])


def parts(prob, loc, scale, threshold, radius, max_det):
    """nms_candidates of every image.  -> (counts int32 [n, J], dets float64 [n, J, max_det, 5])."""
    from oracle.multiperson import nms_candidates

    both = [nms_candidates(prob[b], loc[b], scale, threshold, radius, max_det) for b in range(prob.shape[0])]
    return np.stack([c for c, _ in both]), np.stack([d for _, d in both])


def box_poses(prob, loc):
    """boxfuse_ref.box_poses of the restricted case's boxes on a one-member pyramid (1.0,).  -> float64 [5, 5, J]."""
    import boxfuse_ref as BF

    return BF.box_poses(prob, loc, BOXES, BOX_SCALES, 1.0)


def rounds_to_itself(a):
    """True when every value of `a` survives float16 and bfloat16 (NaN stays NaN, the sign of a zero stays)."""
    import torch

    a = np.array(a, np.float32)  # (a copy: the cases are read-only)
    half = a.astype(np.float16).astype(np.float32)
    bf = torch.from_numpy(a).to(torch.bfloat16).to(torch.float32).numpy()
    same = lambda x: np.array_equal(x.view(np.uint32)[~np.isnan(a)], a.view(np.uint32)[~np.isnan(a)]) and np.isnan(x[np.isnan(a)]).all()  # noqa: E731
    return same(half) and same(bf)

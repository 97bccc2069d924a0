"""Plain-loop float64 restatement of stage D of the people assembly, the completion pass (test helper, never on the product path).

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn stops at the maps, so like stages B and C (tests/people_ref.py) the
rule is this project's own.  What is restated here is its definition in include/deepcut_hip.h (dc_complete_params), on top of
oracle/multiperson.py: the position a cell stands for, the refinement of a cell with `loc_pred`, the prediction of a regression edge.
Small cases only."""
import math

import numpy as np

import people_ref as R
from oracle import multiperson as M

DEFAULTS = dict(fill_threshold=0.25, fill_radius=2, min_support=2)


def _next_at(nxt, row, col):
    """The `next_pred` values [2E] at one cell: from a map [2E, h, w], or from a dict {(row, col): values} (the sparse path: the head
    evaluated at the held candidates' cells only)."""
    if isinstance(nxt, dict):
        return nxt[row, col]
    return nxt[:, row, col]


def complete(dets, people, cand, prob, loc, nxt, edges, mean=None, std=None, scale=1.0, radius=1, fill_threshold=0.25, fill_radius=2,
             min_support=2, items=None):
    """Stage D on ONE image.  dets [J, MD, 5] (stage A), people [m, J, 3] and cand [m, J] (stage C, after the min_joints drop), prob
    [J, h, w], loc [2J, h, w], nxt: see _next_at -> (people, cand) completed: copies, cand == -2 where a joint was filled.

    items (a list, optional) receives one dict per (person q, missing joint j): "q", "j", "support", "e" (None without enough
    predictors), "margin" = the smaller distance of e_x * scale / 8 and e_y * scale / 8 to an integer (inf where e was never floored),
    "cell" = the chosen (row, col) or None, "why" = what left the joint missing, or None."""
    people, cand = np.array(people, np.float64), np.array(cand, np.int32)
    m, J = cand.shape
    h, w = prob.shape[1:]
    E = np.asarray(edges).reshape(-1, 2).shape[0]
    mean = np.zeros((E, 2)) if mean is None else np.asarray(mean, np.float64).reshape(E, 2)
    std = np.ones((E, 2)) if std is None else np.asarray(std, np.float64).reshape(E, 2)
    lut = R.edge_table(edges)
    thr = float(np.float32(fill_threshold))  # the C structure carries it as a float
    held = cand.copy()  # stage C's: fills are neither predictors nor exclusions
    for q in range(m):
        for j in range(J):
            if held[q, j] >= 0:
                continue
            item = dict(q=q, j=j, support=0, e=None, margin=math.inf, cell=None, why=None)
            if items is not None:
                items.append(item)
            # 1. predictors, a ascending
            sx, sy, n = 0.0, 0.0, 0
            for a in range(J):
                l = lut.get((a, j))
                if held[q, a] < 0 or l is None:
                    continue
                row, col = int(dets[a, held[q, a], 3]), int(dets[a, held[q, a], 4])
                v = _next_at(nxt, row, col)
                sx += (col * 8.0 + 4.0 + float(v[2 * l]) * float(std[l, 0]) + float(mean[l, 0])) / scale
                sy += (row * 8.0 + 4.0 + float(v[2 * l + 1]) * float(std[l, 1]) + float(mean[l, 1])) / scale
                n += 1
            item["support"] = n
            if n < min_support or n == 0:
                item["why"] = "support"
                continue
            # 2. the expected position
            ex, ey = sx / n, sy / n
            item["e"] = (ex, ey)
            if not (math.isfinite(ex) and math.isfinite(ey)):
                item["why"] = "not finite"
                continue
            # 3. the window
            gx, gy = ex * scale / 8.0, ey * scale / 8.0
            item["margin"] = min(abs(gx - round(gx)), abs(gy - round(gy)))
            col0, row0 = math.floor(gx), math.floor(gy)
            r_lo, r_hi = max(row0 - fill_radius, 0), min(row0 + fill_radius, h - 1)
            c_lo, c_hi = max(col0 - fill_radius, 0), min(col0 + fill_radius, w - 1)
            if r_lo > r_hi or c_lo > c_hi:
                item["why"] = "off the map"
                continue
            # 4. somebody's peak
            taken = [(int(dets[j, held[p, j], 3]), int(dets[j, held[p, j], 4])) for p in range(m) if held[p, j] >= 0]
            best = None
            for row in range(r_lo, r_hi + 1):
                for col in range(c_lo, c_hi + 1):
                    if any(max(abs(row - tr), abs(col - tc)) <= radius for tr, tc in taken):
                        continue
                    # 5. row-major order: `>` keeps the first of equal scores, and nothing compares true with a NaN
                    v = float(prob[j, row, col])
                    if v >= thr and (best is None or v > best[0]):
                        best = (v, row, col)
            if best is None:
                item["why"] = "below fill_threshold"
                continue
            v, row, col = best
            item["cell"] = (row, col)
            people[q, j] = ((col * M.STRIDE + 0.5 * M.STRIDE + float(loc[2 * j, row, col]) * M.LOCREF) / scale,
                            (row * M.STRIDE + 0.5 * M.STRIDE + float(loc[2 * j + 1, row, col]) * M.LOCREF) / scale, v)
            cand[q, j] = -2
    return people, cand


# ---- the planted scene of tests/test_complete_host.py and tests/test_gpu_complete.py ----------------------------------------------
LOWERED = ((0, 3), (0, 9), (1, 5))  # (person, joint): peaks lowered below the assembly's threshold, above fill_threshold
ASSEMBLY = dict(threshold=0.5, radius=1, max_det=8, max_cost=20.0, seed_threshold=0.55, max_people=32, min_joints=2)
FILL = dict(fill_threshold=0.25, fill_radius=2, min_support=2)
_STATS = np.random.RandomState(5)
MEAN, STD = _STATS.randn(182, 2) * 15, _STATS.uniform(4, 30, (182, 2))  # as tests/test_gpu_people.py


def cell_of(xy, scale=1.0):
    return int(xy[1] * scale // M.STRIDE), int(xy[0] * scale // M.STRIDE)


def lowered_scene(sixteen_bit=False, edges=None, lowered=LOWERED, h=25, w=33):
    """people_ref.planted_scene at 25 x 33 cells with the score peaks of `lowered` set to 0.3125 (exact in every element type).
    -> dict: edges, prob, loc, nxt, joints [3, J, 2], cells {(person, joint): (row, col)}."""
    edges = R.all_pairs_edges() if edges is None else edges
    prob, loc, nxt, joints, strays = R.planted_scene(h, w, edges, MEAN, STD, 1.0, 14, sixteen_bit)
    cells = {(q, j): cell_of(joints[q, j]) for q in range(3) for j in range(14)}
    for q, j in lowered:
        r, c = cells[q, j]
        assert prob[j, r, c] == np.float32((0.875, 0.75, 0.625)[q])
        prob[j, r, c] = 0.3125
    return dict(edges=edges, prob=prob, loc=loc, nxt=nxt, joints=joints, cells=cells)


def assemble_scene(sc, **over):
    """Stages A to C of the restatement on a scene's maps -> (dets, people, cand)."""
    q = dict(ASSEMBLY, **over)
    counts, dets, cost = R.pair_costs(sc["prob"], sc["loc"], sc["nxt"], sc["edges"], 1.0, q["threshold"], q["radius"], q["max_det"], MEAN, STD)
    people, cand = R.assemble(counts, dets, cost, q["max_cost"], q["seed_threshold"], q["max_people"], q["min_joints"])
    return dets, people, cand


def complete_scene(sc, dets, people, cand, items=None, **over):
    """Stage D of the restatement on a scene's maps."""
    f = dict(FILL, **over)
    return complete(dets, people, cand, sc["prob"], sc["loc"], sc["nxt"], sc["edges"], MEAN, STD, 1.0, ASSEMBLY["radius"], items=items, **f)


def smallest_margin(items):
    """The smallest distance of any e * scale / 8 to an integer over the items whose window was placed."""
    return min([it["margin"] for it in items] + [math.inf])

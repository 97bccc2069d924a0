"""Step 4' of the tracking rule (include/deepcut_hip.h, dc_tracker_update): the optimal assignment of a frame's people to a slot's live
tracks, restated in float64 with plain loops.  PARITY UNPINNED BY THE REFERENCE: the reference stops at the maps and has no tracker; what
is restated here is this project's own definition, and the rule is the procedure itself, scan order included.  No import from the
package under test.

    pairs = assign(D, live, n, max_dist)                   # step 4' alone -> {place: person}
    ids, place = associate(slot, D, people, n, P, prm)     # steps 4', 5-7 on a given D (the tests hand it the device's own)

Steps 5-7 are track_ref's, not copied: track_ref.associate is handed a matrix that keeps D at the chosen pairs and is +inf elsewhere, on
which greedy matching returns exactly those pairs."""
import numpy as np

import track_ref as TR

INF = float("inf")


def assign(D, live, n, max_dist, count=None):
    """D [T, P]; live [T] (as of the start of the update); the frame's people are q < n -> {place: person} of the matched pairs.
    count (a dict, optional): "trips" receives the number of trips of the inner loop."""
    rows = [i for i in range(len(live)) if live[i]]  # row r = 1..R is place rows[r - 1]
    R = len(rows)
    m = n + R
    max_dist = float(max_dist)

    # C[r][c]: a real column holds D where `D <= max_dist` is true (NaN <= x is false: forbidden), a dummy column max_dist for every row
    C = [None] + [[None] + [d if d <= max_dist else INF for d in (float(D[i, q]) for q in range(n))] + [max_dist] * R for i in rows]
    u = [0.0] * (R + 1)
    v = [0.0] * (m + 1)
    p = [0] * (m + 1)
    way = [0] * (m + 1)
    trips = 0
    for r in range(1, R + 1):
        p[0] = r
        j0 = 0
        minv = [INF] * (m + 1)
        used = [False] * (m + 1)
        while True:
            trips += 1
            used[j0] = True
            i0 = p[j0]
            delta = INF
            j1 = None
            for j in range(1, m + 1):
                if used[j]:
                    continue
                cur = (C[i0][j] - u[i0]) - v[j]
                if cur < minv[j]:
                    minv[j] = cur
                    way[j] = j0
                if minv[j] < delta:
                    delta = minv[j]
                    j1 = j
            for j in range(m + 1):
                if used[j]:
                    u[p[j]] += delta
                    v[j] -= delta
                else:
                    minv[j] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while True:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
            if j0 == 0:
                break
    if count is not None:
        count["trips"] = count.get("trips", 0) + trips
    return {rows[p[c] - 1]: c - 1 for c in range(1, n + 1) if p[c] != 0}


def total(D, live, pairs, max_dist):
    """What step 4' minimises: the sum of D over the matched pairs + max_dist * (the unmatched live tracks)."""
    return sum(float(D[i, q]) for i, q in pairs.items()) + float(max_dist) * (sum(1 for x in live if x) - len(pairs))


def associate(slot, D, people, n, P, prm, count=None):
    """Steps 4', 5, 6, 7 on the distances D [T, P]; the slot is updated in place -> (ids int64 [P], place int32 [P])."""
    pairs = assign(D, slot.live, n, prm["max_dist"], count)
    chosen = np.full((slot.T, P), INF, np.float64)
    for i, q in pairs.items():
        chosen[i, q] = D[i, q]
    return TR.associate(slot, chosen, people, n, P, prm)


def update(slot, people, n, P, prm, count=None):
    """Steps 1-3, 4', 5-7 -> (ids, place, D)."""
    people = np.asarray(people, np.float64)
    D = TR.distances(slot, people, n, P, prm)
    ids, place = associate(slot, D, people, n, P, prm, count)
    return ids, place, D

"""Step 8 of the tracking rule of include/deepcut_hip.h (dc_tracker_update: smoothed poses that bridge short gaps) restated in float64
with plain loops, on top of track_ref.py's slots.  PARITY UNPINNED BY THE REFERENCE, like the rest of the tracker: the reference stops
at the maps, so there is no reference output to hold the rule to; what is restated here is this project's own definition.  No import
from the package under test.

    prm = params(min_cutoff, beta, d_cutoff, max_hold)
    filt = Filters(T, J)                                         # every filter empty
    before = snapshot(slot)                                      # BEFORE steps 1-7 of the image (track_ref.update / associate)
    ids, place = track_ref.associate(slot, D, people, n, P, tprm)
    smooth, src = step8(filt, before, slot, people, n, P, ids, place, tprm["min_size"], prm, cases)

`cases` (a dict, optional) counts which branch of the rule every item took, so that a test can assert that its scene has them all.
"""
import numpy as np

TWO_PI = 6.283185307179586
# the placeholder parameters of the Python layer (SMOOTH_DEFAULTS), NOT TUNED ON REAL VIDEO
PLACEHOLDERS = {"min_cutoff": 0.1, "beta": 4.0, "d_cutoff": 0.03, "max_hold": 3}
CASES = ("8a_first", "8a_second", "8a_running", "8a_bridged", "8a_expired", "8a_nothing", "8a_born", "8b_aged", "8b_expired", "8b_freed",
         "8c_untracked", "8c_beyond")


def params(min_cutoff=0.1, beta=4.0, d_cutoff=0.03, max_hold=3):
    return {"min_cutoff": float(min_cutoff), "beta": float(beta), "d_cutoff": float(d_cutoff), "max_hold": int(max_hold)}


def A(fc, dt):
    r = (TWO_PI * fc) * dt
    return r / (r + 1.0)


class Filters(object):
    """The filters of one slot: per place and joint fx, fy, dx, dy, fs, gap, n; all empty (n = 0)."""

    def __init__(self, T, J):
        self.T, self.J = int(T), int(J)
        self.reset()

    def reset(self):
        T, J = self.T, self.J
        self.fx, self.fy = np.zeros((T, J)), np.zeros((T, J))
        self.dx, self.dy = np.zeros((T, J)), np.zeros((T, J))
        self.fs = np.zeros((T, J))
        self.gap = [[0] * J for _ in range(T)]
        self.n = [[0] * J for _ in range(T)]


def snapshot(slot):
    """What step 8 needs to know of the slot as it was before the image: which places were live, and with which id."""
    return list(slot.live), list(slot.id)


def person_size(pose, min_size):
    """Step 1 on a pose: max(min_size, the larger extent over the held joints)."""
    xs = [float(p[0]) for p in pose if p[2] > 0]
    ys = [float(p[1]) for p in pose if p[2] > 0]
    s = float(min_size)
    if xs:
        s = max(s, max(max(xs) - min(xs), max(ys) - min(ys)))
    return s


def step8(filt, before, slot, people, n, P, ids, place, min_size, prm, cases=None):
    """-> (smooth float64 [P, J, 3], src int32 [P, J]); the filters are updated in place.  `slot` is the slot AFTER steps 1-7."""
    T, J = filt.T, filt.J
    live_before, id_before = before
    people = np.asarray(people, np.float64)
    smooth = np.zeros((P, J, 3), np.float64)
    src = np.zeros((P, J), np.int32)

    def count(k, by=1):
        if cases is not None:
            cases[k] = cases.get(k, 0) + by

    count("8c_beyond", (P - n) * J)
    touched = set()
    for q in range(n):
        i = int(place[q])
        if i < 0:  # 8c
            for j in range(J):
                smooth[q, j] = people[q, j]
                src[q, j] = 1 if people[q, j, 2] > 0 else 0
            count("8c_untracked", J)
            continue
        touched.add(i)
        born = not (live_before[i] and id_before[i] == int(ids[q]))  # ids are never reused: the same id is the same track
        if born:
            for j in range(J):
                filt.n[i][j] = 0
            count("8a_born", J)
        s = person_size(people[q], min_size)
        for j in range(J):
            px, py, ps = float(people[q, j, 0]), float(people[q, j, 1]), float(people[q, j, 2])
            if ps > 0:
                if filt.n[i][j] == 0:
                    filt.fx[i, j], filt.fy[i, j], filt.dx[i, j], filt.dy[i, j] = px, py, 0.0, 0.0
                    filt.fs[i, j], filt.gap[i][j], filt.n[i][j] = ps, 0, 1
                    smooth[q, j] = (px, py, ps)
                    count("8a_first")
                elif filt.n[i][j] == 1:
                    dt = float(filt.gap[i][j] + 1)
                    filt.dx[i, j] = (px - float(filt.fx[i, j])) / dt
                    filt.dy[i, j] = (py - float(filt.fy[i, j])) / dt
                    filt.fx[i, j], filt.fy[i, j], filt.fs[i, j], filt.gap[i][j], filt.n[i][j] = px, py, ps, 0, 2
                    smooth[q, j] = (px, py, ps)
                    count("8a_second")
                else:
                    dt = float(filt.gap[i][j] + 1)
                    fx, fy, dx, dy = float(filt.fx[i, j]), float(filt.fy[i, j]), float(filt.dx[i, j]), float(filt.dy[i, j])
                    qx, qy = fx + dx * dt, fy + dy * dt
                    ex, ey = px - qx, py - qy
                    a = A(prm["min_cutoff"] + prm["beta"] * ((abs(ex) + abs(ey)) / s), dt)
                    b = A(prm["d_cutoff"], dt)
                    filt.fx[i, j], filt.fy[i, j] = qx + a * ex, qy + a * ey
                    filt.dx[i, j], filt.dy[i, j] = dx + b * (ex / dt), dy + b * (ey / dt)
                    filt.fs[i, j], filt.gap[i][j] = ps, 0
                    smooth[q, j] = (filt.fx[i, j], filt.fy[i, j], ps)
                    count("8a_running")
                src[q, j] = 1
            elif filt.n[i][j] > 0:
                filt.gap[i][j] += 1
                if filt.gap[i][j] > prm["max_hold"]:
                    filt.n[i][j] = 0
                    count("8a_expired")
                else:
                    g = float(filt.gap[i][j])
                    smooth[q, j] = (float(filt.fx[i, j]) + float(filt.dx[i, j]) * g, float(filt.fy[i, j]) + float(filt.dy[i, j]) * g,
                                    float(filt.fs[i, j]))
                    src[q, j] = 2
                    count("8a_bridged")
            else:
                count("8a_nothing")
    for i in range(T):
        if i in touched:
            continue
        if slot.live[i]:  # 8b: live, unmatched, not freed
            for j in range(J):
                if filt.n[i][j] > 0:
                    filt.gap[i][j] += 1
                    if filt.gap[i][j] > prm["max_hold"]:
                        filt.n[i][j] = 0
                        count("8b_expired")
                    else:
                        count("8b_aged")
        else:
            if live_before[i]:
                count("8b_freed")
            for j in range(J):
                filt.n[i][j] = 0
    return smooth, src


def state(filt):
    """What dc_tracker_smooth_state gives: poses [T, J, 3] = (fx + dx * gap, fy + dy * gap, fs) and gap int32 [T, J] where n > 0, zeros
    and -1 elsewhere."""
    T, J = filt.T, filt.J
    poses, gap = np.zeros((T, J, 3), np.float64), np.full((T, J), -1, np.int32)
    for i in range(T):
        for j in range(J):
            if filt.n[i][j] > 0:
                g = float(filt.gap[i][j])
                poses[i, j] = (float(filt.fx[i, j]) + float(filt.dx[i, j]) * g, float(filt.fy[i, j]) + float(filt.dy[i, j]) * g,
                               float(filt.fs[i, j]))
                gap[i, j] = filt.gap[i][j]
    return poses, gap


class Tracked(object):
    """One slot with smoothing, for the tests that need the whole rule on the host: track_ref's steps 1-7 and step 8 behind them."""

    def __init__(self, TR, T, J, tprm, prm):
        self.TR, self.slot, self.filt, self.tprm, self.prm = TR, TR.Slot(T, J), Filters(T, J), tprm, prm

    def update(self, people, n, P, cases=None):
        before = snapshot(self.slot)
        ids, place, _ = self.TR.update(self.slot, people, n, P, self.tprm)
        smooth, src = step8(self.filt, before, self.slot, people, n, P, ids, place, self.tprm["min_size"], self.prm, cases)
        return ids, place, smooth, src

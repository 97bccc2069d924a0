"""The tracking rule of include/deepcut_hip.h (dc_tracker_update) restated in float64 with plain loops: one slot of T track places
updated with the people of one frame.  PARITY UNPINNED BY THE REFERENCE: the reference stops at the maps and has no tracker, so there
is no reference output to hold the rule to; what is restated here is this project's own definition.  No import from the package under
test.

    slot = Slot(T, J); prm = params(J, ...)
    ids, place, D = update(slot, people, n, P, prm)        # steps 1-7
    D = distances(slot, people, n, P, prm)                 # steps 1-3 alone
    ids, place = associate(slot, D, people, n, P, prm)     # steps 4-7 on a given D (the tests hand it the device's own)
"""
import numpy as np

INF = float("inf")


def params(n_joints, sigma=None, max_misses=5, min_common=1, max_dist=1.0, min_size=1.0, motion=1):
    sig = [1.0] * n_joints if sigma is None else [float(v) for v in sigma]
    assert len(sig) == n_joints
    return {"J": int(n_joints), "sigma": sig, "max_misses": int(max_misses), "min_common": int(min_common), "max_dist": float(max_dist),
            "min_size": float(min_size), "motion": int(motion)}


class Slot(object):
    """One sequence: T track places, every one free, and next_id = 0."""

    def __init__(self, T, J):
        self.T, self.J = int(T), int(J)
        self.reset()

    def reset(self):
        T, J = self.T, self.J
        self.live = [False] * T
        self.id = [-1] * T
        self.pose = np.zeros((T, J, 3), np.float64)
        self.vel = np.zeros((T, J, 2), np.float64)
        self.misses = [0] * T
        self.hits = [0] * T
        self.next_id = 0


def distances(slot, people, n, P, prm):
    """Steps 1-3 -> D float64 [T, P]."""
    T, J = slot.T, slot.J
    D = np.full((T, P), INF, np.float64)
    for i in range(T):
        if not slot.live[i]:
            continue
        xs = [float(slot.pose[i, j, 0]) for j in range(J) if slot.pose[i, j, 2] > 0]
        ys = [float(slot.pose[i, j, 1]) for j in range(J) if slot.pose[i, j, 2] > 0]
        s = prm["min_size"]
        if xs:
            s = max(s, max(max(xs) - min(xs), max(ys) - min(ys)))
        m = float(slot.misses[i] + 1)
        for q in range(n):
            total, nc = 0.0, 0
            for j in range(J):
                if not (slot.pose[i, j, 2] > 0 and people[q, j, 2] > 0):
                    continue
                px, py = float(slot.pose[i, j, 0]), float(slot.pose[i, j, 1])
                if prm["motion"] == 1:
                    px = px + float(slot.vel[i, j, 0]) * m
                    py = py + float(slot.vel[i, j, 1]) * m
                dx, dy = px - float(people[q, j, 0]), py - float(people[q, j, 1])
                total += (dx * dx + dy * dy) / ((s * s) * (prm["sigma"][j] * prm["sigma"][j]))
                nc += 1
            if nc >= prm["min_common"] and nc > 0:
                D[i, q] = total / nc
    return D


def associate(slot, D, people, n, P, prm, gaps=None):
    """Steps 4-7 on the distances D [T, P]; the slot is updated in place -> (ids int64 [P], place int32 [P]).

    gaps (a dict, optional) receives how far the run was from deciding otherwise:
      "choice": the smallest difference, over all matching rounds, between the chosen pair and the best pair that choosing it rules out
                (another still open pair of the same track or of the same person);
      "max_dist": the smallest |D - max_dist| over every finite distance of a live track and a person of the frame.
    A perturbation of the distances smaller than half of both cannot change the result."""
    T, J = slot.T, slot.J
    g_choice, g_max = INF, INF
    # 4. pairs above max_dist can never match: the open pairs are listed once, and min() over (D, place, person) IS the tie rule
    pairs = []
    for i in range(T):
        for q in range(n):
            v = float(D[i, q])
            if slot.live[i] and v < INF:
                g_max = min(g_max, abs(v - prm["max_dist"]))
            if slot.live[i] and v <= prm["max_dist"]:
                pairs.append((v, i, q))
    t_match, p_match = {}, {}
    while True:
        still = [c for c in pairs if c[1] not in t_match and c[2] not in p_match]
        if not still:
            break
        v, bi, bq = min(still)
        if gaps is not None:
            for i in range(T):
                if slot.live[i] and i != bi and i not in t_match and float(D[i, bq]) < INF:
                    g_choice = min(g_choice, float(D[i, bq]) - v)
            for q in range(n):
                if q != bq and q not in p_match and float(D[bi, q]) < INF:
                    g_choice = min(g_choice, float(D[bi, q]) - v)
        t_match[bi], p_match[bq] = bq, bi
        pairs = still
    # 5., 6.
    for i in range(T):
        if not slot.live[i]:
            continue
        if i in t_match:
            q = t_match[i]
            m = float(slot.misses[i] + 1)
            for j in range(J):
                if slot.pose[i, j, 2] > 0 and people[q, j, 2] > 0:
                    slot.vel[i, j, 0] = (float(people[q, j, 0]) - float(slot.pose[i, j, 0])) / m
                    slot.vel[i, j, 1] = (float(people[q, j, 1]) - float(slot.pose[i, j, 1])) / m
                else:
                    slot.vel[i, j] = 0.0
            slot.pose[i] = people[q]
            slot.misses[i] = 0
            slot.hits[i] += 1
        else:
            slot.misses[i] += 1
            if slot.misses[i] > prm["max_misses"]:
                slot.live[i] = False
    # 7.
    ids = np.full(P, -1, np.int64)
    place = np.full(P, -1, np.int32)
    for q in range(n):
        if q in p_match:
            ids[q], place[q] = slot.id[p_match[q]], p_match[q]
    free = [i for i in range(T) if not slot.live[i]]
    for q in range(n):
        if q in p_match or not free:
            continue
        i = free.pop(0)
        slot.live[i] = True
        slot.id[i] = slot.next_id
        slot.next_id += 1
        slot.pose[i] = people[q]
        slot.vel[i] = 0.0
        slot.misses[i], slot.hits[i] = 0, 1
        ids[q], place[q] = slot.id[i], i
    if gaps is not None:
        gaps["choice"] = min(gaps.get("choice", INF), g_choice)
        gaps["max_dist"] = min(gaps.get("max_dist", INF), g_max)
    return ids, place


def update(slot, people, n, P, prm, gaps=None):
    """Steps 1-7 -> (ids, place, D)."""
    people = np.asarray(people, np.float64)
    D = distances(slot, people, n, P, prm)
    ids, place = associate(slot, D, people, n, P, prm, gaps)
    return ids, place, D


def state(slot):
    """What dc_tracker_state gives: ids int64 [T], misses int32 [T], hits int32 [T], poses [T, J, 3]; free places -1 / 0 / 0 / zeros."""
    T = slot.T
    ids = np.array([slot.id[i] if slot.live[i] else -1 for i in range(T)], np.int64)
    misses = np.array([slot.misses[i] if slot.live[i] else 0 for i in range(T)], np.int32)
    hits = np.array([slot.hits[i] if slot.live[i] else 0 for i in range(T)], np.int32)
    poses = np.array([slot.pose[i] if slot.live[i] else np.zeros_like(slot.pose[i]) for i in range(T)], np.float64).reshape(T, slot.J, 3)
    return ids, misses, hits, poses

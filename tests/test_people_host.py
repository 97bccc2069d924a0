"""CPU: the host side of the bottom-up people assembly — the pair-statistics reader (dc_pair_stats_read), the argument checks of
`Net.assemble_people`, `pose.people_boxes`, and the restatement of the grouping rule (tests/people_ref.py) on hand-made costs.

PARITY UNPINNED BY THE REFERENCE: eldar/deepcut-cnn has no consumer of `next_pred` (it stops at the maps) and ships no
trained statistics file, so the files read here are written by `write_pair_stats` and the grouping rule pinned here is this
project's own definition (include/deepcut_hip.h), not a reference algorithm."""
import numpy as np
import pytest

import people_ref as R

INF = float("inf")


def _table(seed=0, joints=14):
    rs = np.random.RandomState(seed)
    edges = R.all_pairs_edges(joints)
    return edges, rs.randn(len(edges), 2) * 15, rs.uniform(4, 30, (len(edges), 2))


def _python_parse(path):
    """The format read with nothing but str.split: blocks of '#', name, rows, cols, rows x cols numbers."""
    tok = open(path).read().split()
    mats, p = [], 0
    while p < len(tok) and len(mats) < 3:
        assert tok[p] == "#"
        rows, cols = int(tok[p + 2]), int(tok[p + 3])
        vals = [float(t) for t in tok[p + 4:p + 4 + rows * cols]]
        mats.append(np.array(vals, np.float64).reshape(rows, cols))
        p += 4 + rows * cols
    return mats[0].astype(np.int32) - 1, mats[1], mats[2]


def test_pair_stats_round_trip_182_edges(tmp_path):
    from deepcut_tools import read_pair_stats, write_pair_stats

    edges, mean, std = _table()
    assert edges.shape == (182, 2)
    path = str(tmp_path / "pairs.txt")
    write_pair_stats(path, edges, mean, std)
    e, m, s = read_pair_stats(path)
    assert e.dtype == np.int32 and m.dtype == np.float64 and s.dtype == np.float64
    assert np.array_equal(e, edges) and np.array_equal(m, mean) and np.array_equal(s, std)


def test_c_reader_and_python_parse_agree_exactly(tmp_path):
    from deepcut_tools import read_pair_stats, write_pair_stats

    edges, mean, std = _table(3)
    path = str(tmp_path / "pairs.txt")
    write_pair_stats(path, edges, mean, std)
    with open(path, "a") as f:  # a fourth matrix and free-form spacing: only the first three matrices are used
        f.write("\n#   extra\n 1 3\n 1\t2   3\n")
    got, ref = read_pair_stats(path), _python_parse(path)
    for g, r in zip(got, ref):
        assert g.shape == r.shape and np.array_equal(g, r)
    # hand-written text, numbers in several spellings
    hand = str(tmp_path / "hand.txt")
    open(hand, "w").write("# e\n2 2\n1 2\n2 1\n# m\n2 2 0.5 -1e1\n3 .25\n# s\n2 2\n1 2 3 4.5e0\n")
    got, ref = read_pair_stats(hand), _python_parse(hand)
    for g, r in zip(got, ref):
        assert np.array_equal(g, r)
    assert got[0].tolist() == [[0, 1], [1, 0]] and got[1].tolist() == [[0.5, -10.0], [3.0, 0.25]]


MALFORMED = [
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n", "fewer than three matrices"),
    ("# e\n1 3\n1 2 3\n# m\n1 2\n0 0\n# s\n1 2\n1 1\n", "not E x 2"),
    ("# e\n2 2\n1 2 2 1\n# m\n1 2\n0 0\n# s\n2 2\n1 1 1 1\n", "differing row counts"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n1 2\n1\n", "truncated block"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n", "truncated block"),
    ("# e\n1 2\n0 2\n# m\n1 2\n0 0\n# s\n1 2\n1 1\n", "class id"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n1 2\n1 0\n", "standard deviation"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n1 2\n-2 1\n", "standard deviation"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n1 2\ninf 1\n", "standard deviation"),
    ("# e\n1 2\n1 2\n# m\n1 2\n0 0\n# s\n1 2\nnan 1\n", "standard deviation"),
    ("e\n1 2\n1 2\n", "expected '# <name>'"),
    ("# e\n1 2\n1 x\n", "not a number"),
]


@pytest.mark.parametrize("text,message", MALFORMED)
def test_malformed_pair_stats_are_refused_by_name(tmp_path, text, message):
    import caffe
    from deepcut_tools import read_pair_stats

    path = str(tmp_path / "bad.txt")
    open(path, "w").write(text)
    with pytest.raises(caffe.DeepcutError) as ei:
        read_pair_stats(path)
    assert ei.value.code == -1 and message in str(ei.value), str(ei.value)  # DC_EINVAL


def test_unreadable_file_and_too_many_edges(tmp_path):
    import caffe
    from deepcut_tools import write_pair_stats

    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.pair_stats_read(str(tmp_path / "absent.txt"))
    assert ei.value.code == -2  # DC_EIO
    edges, mean, std = _table()
    path = str(tmp_path / "pairs.txt")
    write_pair_stats(path, edges, mean, std)
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.pair_stats_read(path, max_edges=100)
    assert ei.value.code == -1 and "182 edges" in str(ei.value) and "max_edges = 100" in str(ei.value)
    assert caffe.pair_stats_read(path, max_edges=182)[0].shape == (182, 2)


# ---- the restated assembly on hand-made costs --------------------------------------------------------------------------------------
def _scene(J, MD, groups):
    """groups[q][j] = candidate index person q holds of joint j (or -1).  Scores descend with the person number, so candidate
    lists are in person order unless a test says otherwise.  Cost: 1 + 0.01*(a + c) inside a person, 50 + ... across people."""
    counts = np.zeros(J, np.int32)
    dets = np.zeros((J, MD, 5), np.float64)
    for q, g in enumerate(groups):
        for j, i in enumerate(g):
            if i >= 0:
                counts[j] = max(counts[j], i + 1)
                dets[j, i, :3] = (100.0 * q + j, 10.0 * j + q, 0.9 - 0.1 * q)
    cost = np.full((J, J, MD, MD), INF, np.float64)
    for qa, ga in enumerate(groups):
        for qc, gc in enumerate(groups):
            for a, i in enumerate(ga):
                for c, k in enumerate(gc):
                    if a != c and i >= 0 and k >= 0:
                        cost[a, c, i, k] = (1.0 if qa == qc else 50.0 + 3.0 * abs(qa - qc)) + 0.01 * (a + c)
    return counts, dets, cost


@pytest.mark.parametrize("groups", [
    [[0, 0, 0, 0], [1, 1, 1, 1]],
    [[0, 1, 0, 2], [1, 0, 2, 1], [2, 2, 1, 0]],          # three people, candidate lists shuffled per joint
    [[0, 0, 0, 0], [1, -1, 1, 1], [2, 1, 2, 2]],          # person 1 has no joint 1
])
def test_restated_assembly_returns_the_planted_grouping(groups):
    J, MD = 4, 4
    counts, dets, cost = _scene(J, MD, groups)
    gaps = {}
    people, cand = R.assemble(counts, dets, cost, max_cost=10.0, seed_threshold=0.5, gaps=gaps)
    # people are created in the order joint 0's candidates are listed
    order = sorted(range(len(groups)), key=lambda q: groups[q][0])
    assert cand.tolist() == [groups[q] for q in order]
    for row, q in zip(people, order):
        for j in range(J):
            assert row[j].tolist() == (dets[j, groups[q][j], :3].tolist() if groups[q][j] >= 0 else [0.0, 0.0, 0.0])
    assert gaps["choice"] >= 40 and gaps["max_cost"] >= 8
    # symmetric tensor by construction, as the device writes it
    assert np.array_equal(cost, cost.transpose(1, 0, 3, 2))


def test_restated_assembly_rules():
    J, MD = 3, 3
    counts, dets, cost = _scene(J, MD, [[0, 0, 0], [1, 1, 1]])
    # a tie: both people are equally near candidate 0 of joint 1, and person 0 is equally near both candidates -> lower p, then lower i
    cost[0, 1, :2, :2] = 2.0
    cost[1, 0, :2, :2] = 2.0
    people, cand = R.assemble(counts, dets, cost, 10.0, 0.5)
    assert cand[:, 1].tolist() == [0, 1]
    # max_cost below every link: everybody is a seed of one joint, in joint order then list order; min_joints drops them all
    people, cand = R.assemble(counts, dets, cost, 0.5, 0.5)
    assert cand.tolist() == [[0, -1, -1], [1, -1, -1], [-1, 0, -1], [-1, 1, -1], [-1, -1, 0], [-1, -1, 1]]
    assert R.assemble(counts, dets, cost, 0.5, 0.5, min_joints=2)[1].shape == (0, 3)
    # max_people caps the seeds, later ones are ignored
    assert R.assemble(counts, dets, cost, 0.5, 0.5, max_people=3)[1].tolist() == [[0, -1, -1], [1, -1, -1], [-1, 0, -1]]
    # a seed threshold above person 1's scores (0.8): its candidates join nobody and start nobody
    people, cand = R.assemble(counts, dets, cost, 10.0, 0.85)
    assert cand.tolist() == [[0, 0, 0]]
    # joint order: starting from joint 2
    people, cand = R.assemble(counts, dets, _scene(J, MD, [[0, 0, 0], [1, 1, 1]])[2], 10.0, 0.5, joint_order=[2, 0, 1])
    assert cand.tolist() == [[0, 0, 0], [1, 1, 1]]
    # the mean runs over finite costs only: an infinite pair cost (no edge between joints 0 and 2) is left out, not propagated
    c2 = _scene(J, MD, [[0, 0, 0], [1, 1, 1]])[2]
    c2[0, 2] = c2[2, 0] = INF
    assert R.assemble(counts, dets, c2, 10.0, 0.5)[1].tolist() == [[0, 0, 0], [1, 1, 1]]
    # no candidates at all
    people, cand = R.assemble(np.zeros(J, np.int32), dets, cost, 10.0, 0.5)
    assert people.shape == (0, J, 3) and cand.shape == (0, J)


def test_pair_cost_restatement_on_a_tiny_map():
    """Two joints, one candidate each, both directions: the cost is scale * the mean of the two prediction errors; one direction
    only: that direction's error alone; duplicates: the lowest index counts."""
    from oracle import multiperson as M

    h, w = 4, 5
    prob = np.zeros((2, h, w), np.float32)
    loc = np.zeros((4, h, w), np.float32)
    nxt = np.zeros((4, h, w), np.float32)
    prob[0, 1, 1] = 0.9  # joint 0 at (12, 12)
    prob[1, 2, 3] = 0.8  # joint 1 at (28, 20)
    nxt[0:2, 1, 1] = (19.0, 8.0)   # edge 0 = (0, 1): predicts (31, 20), 3 px off
    nxt[2:4, 2, 3] = (-16.0, -4.0)  # edge 1 = (1, 0): predicts (12, 16), 4 px off
    for scale in (1.0, 0.5):
        counts, dets, cost = R.pair_costs(prob, loc, nxt, [(0, 1), (1, 0)], scale, 0.5, 1, 2)
        assert counts.tolist() == [1, 1]
        assert cost[0, 1, 0, 0] == cost[1, 0, 0, 0] == 3.5
        assert np.isinf(cost[0, 0]).all() and np.isinf(cost[0, 1, 1:]).all() and np.isinf(cost[0, 1, :, 1:]).all()
        _, _, one = R.pair_costs(prob, loc, nxt, [(0, 1), (0, 1)], scale, 0.5, 1, 2)
        assert one[0, 1, 0, 0] == one[1, 0, 0, 0] == 3.0
    nxt2 = np.concatenate([nxt, np.zeros((2, h, w), np.float32)])
    nxt2[4:6, 1, 1] = (100.0, 100.0)  # edge 2 = (0, 1) again: ignored
    _, _, dup = R.pair_costs(prob, loc, nxt2, [(0, 1), (1, 0), (0, 1)], 1.0, 0.5, 1, 2)
    assert dup[0, 1, 0, 0] == 3.5
    assert M.STRIDE == 8


# ---- Python surface ------------------------------------------------------------------------------------------------------------------
def test_people_boxes():
    from pose import people_boxes

    people = np.zeros((3, 4, 3))
    people[0, :3] = [(10.2, 20.7, 0.9), (30.0, 25.0, 0.8), (12.0, 60.5, 0.7)]    # joint 3 missing: (0, 0, 0) must not pull the box
    people[1, 1] = (98.5, 3.0, 0.6)                                              # one joint near the border
    boxes = people_boxes(people, (80, 100, 3), 5)
    assert boxes.dtype == np.int32 and boxes.shape == (3, 4)
    assert boxes[0].tolist() == [5, 15, 36, 67]
    assert boxes[1].tolist() == [93, 0, 100, 9]
    assert boxes[2].tolist() == [0, 0, 100, 80]     # nobody assigned: the whole image
    assert people_boxes(people[:1], (80, 100), 0)[0].tolist() == [10, 20, 31, 62]
    assert people_boxes(np.zeros((0, 4, 3)), (80, 100), 5).shape == (0, 4)
    import caffe

    b, _, _ = caffe.check_boxes((80, 100, 3), boxes)   # exactly what the box entry accepts
    assert np.array_equal(b, boxes)
    with pytest.raises(ValueError):
        people_boxes(np.zeros((4, 3)), (80, 100), 5)


def test_assemble_people_refuses_bad_arguments_without_a_gpu():
    import ctypes as C

    import caffe
    import caffe.pycaffe as pc
    from deepcut_tools import deepercut_prototxt

    net = caffe.Net(deepercut_prototxt(152, 64, 64), caffe.TEST, from_text=True)
    edges = R.all_pairs_edges()
    ok = dict(edges=edges, max_cost=20.0, seed_threshold=0.5)
    for kw, word in [
        (dict(ok, edges=None), "edges"),
        (dict(ok, edges=edges[:, :1]), "E x 2"),
        (dict(ok, edges=np.where(edges == 13, 14, edges)), "outside [0, 14)"),
        (dict(ok, edges=np.where(edges == 0, -1, edges)), "outside [0, 14)"),
        (dict(ok, edges=np.vstack([edges[:181], [[4, 4]]])), "to itself"),
        (dict(ok, edges=edges[:100]), "100 edges"),
        (dict(ok, joint_order=list(range(13))), "permutation"),
        (dict(ok, joint_order=[0] * 14), "permutation"),
        (dict(ok, joint_order=list(range(1, 15))), "permutation"),
        (dict(ok, max_det=65), "max_det"),
        (dict(ok, max_det=0), "max_det"),
        (dict(ok, max_people=257), "max_people"),
        (dict(ok, min_joints=15), "min_joints"),
        (dict(ok, max_cost=float("inf")), "max_cost"),
        (dict(ok, scale=0.0), "scale"),
        (dict(ok, threshold=-0.1), "threshold"),
        (dict(ok, radius=65), "radius"),
        (dict(ok, mean=np.zeros((181, 2))), "mean"),
        (dict(ok, std=np.zeros((182, 2))), "std"),
    ]:
        with pytest.raises(ValueError) as ei:
            net.assemble_people(**kw)
        assert word in str(ei.value), (word, str(ei.value))
    # well-formed arguments pass the Python checks and reach the library, which has no CPU path
    with pytest.raises(caffe.DeepcutError) as ei:
        net.assemble_people(**ok)
    # DC_EDEVICE / DC_ENOCPU; in a session whose thread is in GPU mode on a machine with a device: no forward has run
    assert ei.value.code in (-5, -6) or "run forward() first" in str(ei.value)
    # the library refuses the same things on its own, before any device work (a C caller has no Python checks in front)
    L = pc._lib
    count = np.zeros(1, np.int32)
    people = np.zeros((1, 32, 14, 3))
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(q, e, order=None):
        e = np.ascontiguousarray(e, np.int32)
        o = None if order is None else vp(np.ascontiguousarray(order, np.int32))
        return L.dc_net_assemble_people(net._h, C.byref(q), e.shape[0], vp(e), None, None, o, vp(count), vp(people), None, None)

    good = lambda **kw: pc.AssembleParams(**dict(dict(scale=1.0, threshold=0.1, radius=1, max_det=16, max_cost=20.0, seed_threshold=0.5,  # noqa: E731
                                                      max_people=32, min_joints=1), **kw))
    for q, e, order, word in [
        (good(max_det=65), edges, None, b"max_det"),
        (good(max_people=0), edges, None, b"max_people"),
        (good(min_joints=0), edges, None, b"min_joints"),
        (good(max_cost=-1.0), edges, None, b"max_cost"),
        (good(scale=-1.0), edges, None, b"scale"),
        (good(), np.where(edges == 13, 14, edges), None, b"outside [0, 14)"),
        (good(), np.vstack([edges[:181], [[4, 4]]]), None, b"to itself"),
        (good(), edges, [0] * 14, b"permutation"),
    ]:
        assert call(q, e, order) == -1 and word in L.dc_last_error(), L.dc_last_error()
    assert call(good(), edges) in (-5, -6) or b"run forward() first" in L.dc_last_error()


def test_estimate_people_refuses_a_net_without_next_pred_and_leaves_it_alone():
    import caffe
    from deepcut_tools import deepercut_prototxt
    from pose import estimate_people

    net = caffe.Net(deepercut_prototxt(152, 64, 64), caffe.TEST, from_text=True)
    net.set_outputs(["loc_pred", "prob"])
    stats = (R.all_pairs_edges(), None, None)
    with pytest.raises(ValueError) as ei:
        estimate_people(np.zeros((64, 64, 3), np.uint8), None, None, stats, net=net)
    assert "next_pred" in str(ei.value)
    assert net.wanted_outputs == ["loc_pred", "prob"]

"""Stage E of the people assembly (dedupe) without a GPU: the float64 restatement of tests/dedupe_ref.py on the crafted scenes of
tests/dedupe_scenes.py, held to survivors derived by hand; the condition on those scenes that makes them a fair test of the device
(every decision at least 1e-9 away from max_dist, or an intended exact pair); and the refusals of dc_net_set_dedupe /
dc_group_set_dedupe / dc_dedupe_people, which need no device.

Why 1e-9 is enough: the device's double arithmetic may contract multiply-adds and so differ from these loops by roughly
(2J + 4) * 2^-53 relative, eight orders of magnitude less.  It is a condition on the inputs, not a tolerance on a result.

PARITY UNPINNED BY THE REFERENCE: the reference repository stops at the maps; the rule (include/deepcut_hip.h, dc_dedupe_params) is
this project's own, like stages B to D and the tracker."""
import ctypes as C

import numpy as np
import pytest

import dedupe_ref as E
import dedupe_scenes as S
import people_ref as R


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_the_restatement_gives_the_survivors_derived_by_hand(name):
    sc = S.scene(name)
    n_out, people, cand, kept_from, by, recs = S.reference(name)
    nb, P = sc["people"].shape[:2]
    for b in range(nb):
        n, kept = int(sc["n"][b]), sc["kept"][b]
        assert n_out[b] == len(kept)
        assert kept_from[b, :len(kept)].tolist() == kept and (kept_from[b, len(kept):] == -1).all()
        want_by = [sc["by"][b].get(q, -1) for q in range(n)]
        assert by[b, :n].tolist() == want_by and (by[b, n:] == -1).all()
        if "people_out" in sc:
            exp_p, exp_c = sc["people_out"][b], sc["cand_out"][b]
        else:
            exp_p = sc["people"][b, kept]
            exp_c = sc["cand"][b, kept] if sc["cand"] is not None else np.where(exp_p[..., 2] > 0, 0, -1)
        assert people[b, :len(kept)].tobytes() == np.ascontiguousarray(exp_p, np.float64).tobytes()
        assert np.array_equal(cand[b, :len(kept)], exp_c)
        assert (people[b, len(kept):] == 0).all() and (cand[b, len(kept):] == -1).all()
        # a suppressed person suppresses nobody, and a killer ranks before its victim
        rank = recs[b]["rank"]
        for q, k in sc["by"][b].items():
            assert by[b, k] == -1 and rank[k] < rank[q]


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_every_decision_of_the_scenes_is_far_from_max_dist_or_an_intended_exact_pair(name):
    sc = S.scene(name)
    recs = S.reference(name)[5]
    for b, rec in enumerate(recs):
        m = E.check_margins(rec, sc["params"]["max_dist"], sc["params"]["min_common"], sc["exact"][b])
        print("%s image %d: %d pairs, smallest margin %.3g (the restatement's own, intended pairs included: %.3g)"
              % (name, b, len(rec["pairs"]), m, rec["margin"]))
        assert m >= 1e-9


def test_the_restatement_reports_every_pair_and_its_margin():
    sc = S.scene("a_chain")
    rec = S.reference("a_chain")[5][0]
    pairs = {(a, b): (ra, rb, nc, D, sim, cons) for a, b, ra, rb, nc, D, sim, cons in rec["pairs"]}
    assert pairs == {(0, 1): (0, 1, 1, 0.25, True, True), (0, 2): (0, 2, 1, 1.0, False, True), (1, 2): (1, 2, 1, 0.25, True, False)}
    assert rec["margin"] == 0.5  # |0.25 - 0.5| / 0.5
    tie = S.reference("b_tie")[5]
    assert [r["margin"] for r in tie] == [0.0, 0.0, 0.0] and [r["pairs"][0][4] for r in tie] == [1, 2, 4]
    above = S.reference("b_one_ulp_above")[5]
    assert all(0 < r["margin"] < 1e-15 and not r["pairs"][0][6] for r in above)
    assert sc["params"]["max_dist"] == 0.5


def test_absorbed_joints_change_no_decision():
    """The third person of scene (g) is similar to A once A holds B's joints: running the rule again on the OUTPUT suppresses it, the rule
    itself, which reads its input only, keeps it."""
    sc = S.scene("g_absorb")
    n_out, people, cand, kept_from, _by, _ = S.reference("g_absorb")
    assert n_out[0] == 2 and kept_from[0, :2].tolist() == [0, 3] and (cand[0, 0] >= 0).all()
    again = E.dedupe_ref(people[0, :2], cand[0, :2], **sc["params"])
    assert again["kept_from"].tolist() == [0] and again["suppressed_by"].tolist() == [-1, 0]


# ---- the setting itself and the argument checks: no device needed ------------------------------------------------------------------
def _net():
    import caffe
    from deepcut_tools import deepercut_prototxt

    return caffe.Net(deepercut_prototxt(152, 64, 64), caffe.TEST, from_text=True)


BAD = [
    (dict(max_dist=-0.5), "max_dist"),
    (dict(max_dist=float("nan")), "max_dist"),
    (dict(max_dist=float("inf")), "max_dist"),
    (dict(min_common=0), "min_common"),
    (dict(min_common=-3), "min_common"),
    (dict(min_size=0.0), "min_size"),
    (dict(min_size=-1.0), "min_size"),
    (dict(min_size=float("nan")), "min_size"),
    (dict(min_size=float("inf")), "min_size"),
    (dict(sigma=[1.0, 0.0, 1.0]), "sigma of joint 1"),
    (dict(sigma=[1.0, 1.0, -2.0]), "sigma of joint 2"),
    (dict(sigma=[float("nan")]), "sigma of joint 0"),
    (dict(sigma=[float("inf")] * 2), "sigma of joint 0"),
    (dict(sigma=[1.0] * 33), "n_sigma"),
]


def _same(a, b):
    if a is None or b is None:
        return a is b
    return all(np.array_equal(a[k], b[k]) if k == "sigma" and a[k] is not None and b[k] is not None else a[k] == b[k] for k in set(a) | set(b))


def test_set_dedupe_in_python_without_a_device():
    import caffe

    D0 = caffe.pycaffe.DEDUPE_DEFAULTS
    net = _net()
    assert net.dedupe is None
    net.dedupe = True
    assert _same(net.dedupe, D0) and net.dedupe is not D0
    sig = [0.5 + j / 16.0 for j in range(14)]
    net.dedupe = dict(max_dist=0.0, min_common=14, min_size=8.0, sigma=sig, absorb=False)
    assert _same(net.dedupe, dict(max_dist=0.0, min_common=14, min_size=8.0, sigma=np.array(sig), absorb=False))
    net.dedupe = dict(min_common=2)  # the others: the defaults
    good = dict(D0, min_common=2)
    assert _same(net.dedupe, good)
    for kw, word in BAD:
        with pytest.raises(caffe.DeepcutError) as ei:
            net.dedupe = kw
        assert ei.value.code == -1 and word in str(ei.value), (kw, str(ei.value))
        assert _same(net.dedupe, good)  # a refused value changes nothing
    with pytest.raises(ValueError) as ei:
        net.dedupe = dict(max_dits=0.3)
    assert "max_dits" in str(ei.value)
    with pytest.raises(TypeError):
        net.dedupe = 0.3
    with pytest.raises(ValueError):
        net.dedupe = dict(min_size="wide")
    # a clone has its net's setting at clone time, and one of its own afterwards
    net.dedupe = dict(sigma=sig, max_dist=0.125)
    c = net.clone()
    assert _same(c.dedupe, net.dedupe) and np.array_equal(c.dedupe["sigma"], sig)
    net.dedupe = None
    assert net.dedupe is None and _same(c.dedupe, dict(D0, sigma=np.array(sig), max_dist=0.125))
    assert net.clone().dedupe is None
    c.dedupe = False
    assert c.dedupe is None
    # a group has a setting of its own
    g = caffe.NetGroup([net, c])
    assert g.dedupe is None
    g.dedupe = dict(absorb=False)
    assert _same(g.dedupe, dict(D0, absorb=False)) and net.dedupe is None and c.dedupe is None
    for kw, word in BAD:
        with pytest.raises(caffe.DeepcutError) as ei:
            g.dedupe = kw
        assert ei.value.code == -1 and word in str(ei.value)
    g.dedupe = None
    assert g.dedupe is None
    # completion is a setting of its own beside it
    net.completion, net.dedupe = True, True
    net.completion = None
    assert net.completion is None and _same(net.dedupe, D0)


def test_a_dedupe_argument_is_refused_before_the_device_and_leaves_the_setting_alone():
    import caffe

    net = _net()
    net.dedupe = dict(min_common=5)
    net.completion = dict(fill_radius=5)
    before, before_c = net.dedupe, net.completion
    edges = R.all_pairs_edges()
    with pytest.raises(caffe.DeepcutError) as ei:
        net.assemble_people(edges=edges, dedupe=dict(min_size=-4.0))
    assert ei.value.code == -1 and "min_size" in str(ei.value)
    assert _same(net.dedupe, before) and net.completion == before_c
    # a good one reaches the library's assembly entry, which has no CPU path; the net's own settings are back afterwards
    with pytest.raises(caffe.DeepcutError) as ei:
        net.assemble_people(edges=edges, dedupe=True, complete=True)
    assert ei.value.code in (-5, -6) or "run forward() first" in str(ei.value)
    assert _same(net.dedupe, before) and net.completion == before_c
    with pytest.raises(caffe.DeepcutError):
        net.assemble_people(edges=edges, dedupe=False)
    assert _same(net.dedupe, before)


def _params(pc, sigma=None, **kw):
    d = dict(enabled=1, max_dist=0.25, min_common=2, min_size=16.0, absorb=1)
    d.update(kw)
    sig = None if sigma is None else np.ascontiguousarray(sigma, np.float64)
    q = pc.DedupeParams(d["enabled"], d["max_dist"], d["min_common"], d["min_size"], None if sig is None else sig.ctypes.data,
                        d.get("n_sigma", 0 if sig is None else sig.shape[0]), d["absorb"])
    return q, sig


def _read(L, get, h, pc):
    out, sig = pc.DedupeParams(9, 9.0, 9, 9.0, None, 9, 9), np.full(32, 9.0)
    assert get(h, C.byref(out), sig.ctypes.data_as(C.c_void_p)) == 0
    return (out.enabled, out.max_dist, out.min_common, out.min_size, out.n_sigma, out.absorb), sig


C_BAD = [
    (dict(max_dist=-1.0), None, b"max_dist"),
    (dict(max_dist=float("nan")), None, b"max_dist"),
    (dict(min_common=0), None, b"min_common"),
    (dict(min_size=0.0), None, b"min_size"),
    (dict(min_size=float("inf")), None, b"min_size"),
    (dict(absorb=2), None, b"absorb"),
    (dict(absorb=-1), None, b"absorb"),
    (dict(n_sigma=3), None, b"sigma"),       # values promised, none given
    (dict(n_sigma=-1), [1.0], b"n_sigma"),
    (dict(n_sigma=33), [1.0] * 33, b"n_sigma"),
    (dict(), [1.0, -1.0], b"sigma of joint 1"),
]


def test_set_dedupe_through_the_c_abi_without_a_device():
    import caffe
    import caffe.pycaffe as pc

    L = pc._lib
    net = _net()
    g = caffe.NetGroup([net, net.clone()])
    for set_, get, h in ((L.dc_net_set_dedupe, L.dc_net_get_dedupe, net._h), (L.dc_group_set_dedupe, L.dc_group_get_dedupe, g._h)):
        got, sig = _read(L, get, h, pc)
        assert got == (0, 0.0, 0, 0.0, 0, 0) and (sig == 0).all()
        q, keep = _params(pc, sigma=[0.5, 2.0, 1.0])
        assert set_(h, C.byref(q)) == 0
        keep[:] = 7.0  # the values were copied: the caller's array may change or go
        got, sig = _read(L, get, h, pc)
        assert got == (1, 0.25, 2, 16.0, 3, 1) and sig[:3].tolist() == [0.5, 2.0, 1.0] and (sig[3:] == 0).all()
        for kw, sigma, word in C_BAD:
            q, keep = _params(pc, sigma=sigma, **kw)
            assert set_(h, C.byref(q)) == -1, kw
            assert word in L.dc_last_error(), (kw, L.dc_last_error())
            assert _read(L, get, h, pc)[0] == (1, 0.25, 2, 16.0, 3, 1)  # a refused value changes nothing
        # a sigma pointer with n_sigma = 0 is "all 1.0", and max_dist = 0 is allowed
        q, keep = _params(pc, sigma=[3.0], n_sigma=0, max_dist=0.0)
        assert set_(h, C.byref(q)) == 0 and _read(L, get, h, pc)[0] == (1, 0.0, 2, 16.0, 0, 1)
        # not enabled: the other fields are not read, and everything reads back as zero
        q, keep = _params(pc, enabled=0, max_dist=-1.0, min_common=0, min_size=-1.0, absorb=5, n_sigma=99)
        assert set_(h, C.byref(q)) == 0
        got, sig = _read(L, get, h, pc)
        assert got == (0, 0.0, 0, 0.0, 0, 0) and (sig == 0).all()
        q, keep = _params(pc)
        assert set_(h, C.byref(q)) == 0 and _read(L, get, h, pc)[0][0] == 1
        assert set_(h, None) == 0  # NULL: off
        assert _read(L, get, h, pc)[0] == (0, 0.0, 0, 0.0, 0, 0)
        assert set_(None, None) == -1 and get(h, None, None) == -1 and get(None, C.byref(q), None) == -1
        out = pc.DedupeParams()
        assert get(h, C.byref(out), None) == 0  # sigma_out may be NULL


def test_dedupe_people_checks_its_arguments_before_any_device_work():
    import caffe.pycaffe as pc

    L = pc._lib
    nb, P, J = 2, 3, 4
    n = np.array([3, 1], np.int32)
    ppl = np.zeros((nb, P, J, 3))
    n_out, out = np.zeros(nb, np.int32), np.zeros_like(ppl)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731

    def call(q, nb=nb, P=P, J=J, n=n, ppl=ppl, n_out=n_out, out=out):
        return L.dc_dedupe_people(None if q is None else C.byref(q), nb, P, J, ptr(n), ptr(ppl), None, ptr(n_out), ptr(out), None, None, None)

    good, _ = _params(pc)
    for kw, sigma, word in C_BAD:
        q, keep = _params(pc, sigma=sigma, **kw)
        assert call(q) == -1 and word in L.dc_last_error(), (kw, L.dc_last_error())
    q, _ = _params(pc, enabled=0, max_dist=-1.0)  # no switch here: the fields are checked whatever `enabled` says
    assert call(q) == -1 and b"max_dist" in L.dc_last_error()
    for kw, word in ((dict(q=None), b"null"), (dict(n=None), b"null"), (dict(ppl=None), b"null"), (dict(n_out=None), b"null"),
                     (dict(out=None), b"null"), (dict(nb=0), b"nb"), (dict(nb=-2), b"nb"), (dict(P=0), b"max_people"), (dict(P=257), b"max_people"),
                     (dict(J=0), b"n_joints"), (dict(J=33), b"n_joints"), (dict(n=np.array([4, 0], np.int32)), b"n_people[0]"),
                     (dict(n=np.array([0, -1], np.int32)), b"n_people[1]")):
        assert call(**dict(dict(q=good), **kw)) == -1, kw
        assert word in L.dc_last_error(), (kw, L.dc_last_error())
    # what only the joints decide is a shape error
    q, keep = _params(pc, sigma=[1.0, 1.0, 1.0])
    assert call(q) == -3 and b"sigma" in L.dc_last_error()
    q, _ = _params(pc, min_common=5)
    assert call(q) == -3 and b"min_common" in L.dc_last_error()
    # everything in order: the call gets as far as the device, which this test does not need
    q, keep = _params(pc, sigma=[1.0] * 4, min_common=4)
    import caffe

    if caffe.device_count() < 1:
        caffe.set_mode_gpu()
        assert call(q) == -5
    caffe.set_mode_cpu()
    assert call(q) == -6 and b"CPU mode" in L.dc_last_error()  # DC_ENOCPU


def test_dedupe_people_in_python_shapes_its_arguments():
    import caffe

    with pytest.raises(ValueError):
        caffe.dedupe_people(np.zeros((2, 3, 4, 2)))
    with pytest.raises(ValueError):
        caffe.dedupe_people(np.zeros((2, 3, 4, 3)), n_people=[3])
    with pytest.raises(ValueError):
        caffe.dedupe_people(np.zeros((2, 3, 4, 3)), cand=np.zeros((2, 3, 5), np.int32))
    with pytest.raises(ValueError):
        caffe.dedupe_people([np.zeros((1, 4, 3)), np.zeros((1, 5, 3))])
    with pytest.raises(ValueError):
        caffe.dedupe_people(np.zeros((1, 1, 4, 3)), dedupe=False)
    with pytest.raises(ValueError):
        caffe.dedupe_people(np.zeros((1, 1, 4, 3)), dedupe=dict(treshold=1))
    assert caffe.dedupe_people([]) == []
    caffe.set_mode_cpu()
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.dedupe_people(np.zeros((1, 1, 4, 3)), dedupe=dict(min_common=9))
    assert ei.value.code == -3
    with pytest.raises(caffe.DeepcutError) as ei:
        caffe.dedupe_people([np.zeros((2, 4, 3)), np.zeros((0, 4, 3))], cand=[np.zeros((2, 4), int), np.zeros((0, 4), int)])
    assert ei.value.code == -6

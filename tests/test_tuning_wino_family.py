"""CPU: deepcut_tools.tune_in_flight tries every timed form of the float32 Winograd kernel that is within the margin, not only the first
`max_candidates`: alone the forms differ by less than the timing's noise (one round of workgroups on any cover), under load a cover of fewer
blocks frees workgroup slots for the other forwards.  Tiles outside the family keep the limit (tests/test_tuning_logic.py)."""
from deepcut_tools import tune_in_flight

from test_tuning_logic import FakeNet


def _run(timed, cost, **kw):
    log = []
    rep = [{"signature": "res4 3x3+w", "tile": timed[0][0], "launches": 36, "timed": timed}]
    nets = [FakeNet(rep, log), FakeNet(rep, log)]
    res = tune_in_flight(nets, lambda: cost[nets[0].report[0]["tile"]], reps=1, **kw)
    assert nets[0].report[0]["tile"] == nets[1].report[0]["tile"]
    return nets[0].report[0]["tile"], log, res


def test_the_mixed_form_is_reached_from_the_fourth_place():
    timed = [("wino_f23_w16", 15.0), ("wino_f23_mix_w16", 15.1), ("wino_f23", 15.2), ("wino_f23_mix", 15.3), ("e64x64", 17.0), ("f128", 40.0)]
    cost = {"wino_f23_w16": 1.00, "wino_f23_mix_w16": 0.99, "wino_f23": 0.97, "wino_f23_mix": 0.95, "e64x64": 0.5, "f128": 0.5}
    tile, log, res = _run(timed, cost)
    assert tile == "wino_f23_mix" and [c[1:3] for c in res["changed"]] == [("wino_f23_w16", "wino_f23"), ("wino_f23", "wino_f23_mix")]
    assert ("res4 3x3+w", "e64x64") not in log and ("res4 3x3+w", "f128") not in log  # a direct tile past the limit, one outside the margin


def test_a_family_member_outside_the_margin_is_not_tried():
    timed = [("wino_f23_5x6", 45.0), ("wino_f23_5x6_w16", 49.0), ("a", 50.0), ("wino_f23", 67.0), ("wino_f23_w16", 72.0)]
    cost = {"wino_f23_5x6": 1.0, "wino_f23_5x6_w16": 1.0, "a": 1.0, "wino_f23": 0.5, "wino_f23_w16": 0.5}
    tile, log, _res = _run(timed, cost)
    assert tile == "wino_f23_5x6" and not [t for _s, t in log if t in ("wino_f23", "wino_f23_w16")]

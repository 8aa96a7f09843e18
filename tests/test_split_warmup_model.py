"""The time split's warm-up rules without a GPU (gnuspeech_amd/csrc/trm_warm.h; include/trm_c_api.h:
trm_batch_set_split_warmup).  tests/_emul/warm_emul.cc puts the header behind a C interface; here both rules are held against
a restatement made in tests/split_warmup_common.py, the default rule against the one the time-split tests have always used
(test_time_split.warm_periods), and the coupled rule -- through the host model of the split arithmetic -- against the oracle on
the parameters the default rule does not cover: mouth and nose reflection filters far from Monet's inside their loops.

What the default rule leaves on those inputs is printed, never asserted: this file does not pin the gap."""
import numpy as np
import pytest

import cases
import golden_io
import parity
import split_warmup_common as W
from test_time_split import RMS_TOL, _emul_split, emul, nrms, warm_periods  # noqa: F401  (emul: a fixture)


@pytest.fixture(scope="module")
def rules():
    return W.warm_emul()


def _fixture_sets():
    return [(n, golden_io.load(n)["params_dict"]) for n in golden_io.CASE_NAMES + golden_io.TRACT_CASE_NAMES + golden_io.TRACT_SLICE_CASE_NAMES]


def _sweep(n=200, seed=23):
    """Parameter sets over the legal ranges of what the rules read: loss, both end filters, the throat low-pass -- at three
    output rates and three tube lengths, so that control period and tube rate move too."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        pd = dict(cases.monet_default_params([44100.0, 22050.0, 16000.0][k % 3]), length=[17.5, 15.0, 12.5][(k // 3) % 3],
                  lossFactor=float(rng.uniform(0.05, 5.0)), mouthCoef=float(rng.uniform(100.0, 9000.0)),
                  noseCoef=float(rng.uniform(100.0, 9000.0)), throatCutoff=float(rng.uniform(50.0, 6000.0)))
        out.append(("sweep %d" % k, pd))
    return out


def test_both_rules_are_what_the_restatement_says(rules):
    for name, pd in _fixture_sets() + _sweep():
        r = W.emul_rules(rules, pd)
        cp = r["controlPeriod"]
        assert cp == W.control_period_of(pd), name
        for rule in ("default", "coupled"):
            samples, periods = r[rule]
            assert periods == W.rule_periods(pd, cp, rule), (name, rule, periods)
            assert periods == (samples + cp - 1) // cp, (name, rule)
        # the default rule is the one the time-split tests have always held the library to
        assert r["default"][1] == warm_periods(pd, cp), name
        # never shorter, in samples as in periods
        assert r["coupled"][0] >= r["default"][0] > 0 and r["coupled"][1] >= r["default"][1], (name, r)


def test_the_loop_pole_is_the_larger_root_and_lies_above_the_filter_and_the_round_trip(rules):
    for c in (0.0, 0.2, 0.5468, 0.9, 0.9819, 0.999):
        for d in (0.95, 0.99, 0.995, 0.9995):
            rho = rules.warm_emul_loop_pole(c, d)
            assert abs(rho - W.loop_pole(c, d)) <= 1e-15
            assert abs(rho * rho - c * rho - d * d * (1.0 - c)) <= 1e-14           # a root of the loop's characteristic equation
            assert rho >= c and rho >= d * d - 1e-15 and rho < 1.0, (c, d, rho)


def test_values_at_monets_defaults_and_on_the_verdict_set(rules):
    r = W.emul_rules(rules, cases.monet_default_params(44100.0))
    assert (r["default"][1], r["coupled"][1]) == (30, 45)
    r = W.emul_rules(rules, W.VERDICT_PD)
    assert r["controlPeriod"] == 79
    assert (r["default"][1], r["coupled"][1]) == (W.VERDICT_WARM["default"], W.VERDICT_WARM["coupled"]) == (16, 189)
    assert r["default"][1] == warm_periods(W.VERDICT_PD, 79)


def test_a_tube_without_loss_never_forgets_under_either_rule(rules):
    for pd in (cases.monet_default_params(44100.0), W.VERDICT_PD, W.DOWN_PD):
        r = W.emul_rules(rules, dict(pd, lossFactor=0.0))
        assert r["default"] == (0, 0) and r["coupled"] == (0, 0)
        assert W.rule_periods(dict(pd, lossFactor=0.0), r["controlPeriod"], "coupled") == 0


def _split_errors(emul, pd, fr, warm, what):
    """The host model of the split arithmetic, cut every SEG periods with `warm`, against the oracle: (count ok, nrms, worst
    control period's nrms)"""
    o = W.oracle_of(pd, fr)
    y, _ = _emul_split(emul, W.O.InputParams.from_dict(pd), fr, W.SEG, warm)
    assert len(y) == o["numberSamples"], (what, len(y), o["numberSamples"])
    r = parity.windowed_error(y, o["samples"], o["maximumSampleValue"], parity.window_length_of(pd))
    return o, y, r


def test_the_verdict_case_meets_the_tolerance_under_the_coupled_rule(emul, rules):
    fr = W.verdict_frames()
    warm = W.emul_rules(rules, W.VERDICT_PD)
    o, y, r = _split_errors(emul, W.VERDICT_PD, fr, warm["coupled"][1], "coupled")
    _, _, rd = _split_errors(emul, W.VERDICT_PD, fr, warm["default"][1], "default")
    print("VERDICT case, S = %d: coupled W = %d nrms %.3g (worst period %.3g); default W = %d nrms %.3g (worst period %.3g)"
          % (W.SEG, warm["coupled"][1], r["nrms"], r["worst_window_nrms"], warm["default"][1], rd["nrms"], rd["worst_window_nrms"]))
    assert nrms(y, o["samples"], o["maximumSampleValue"]) <= RMS_TOL
    parity.check_oracle(y, o, parity.window_length_of(W.VERDICT_PD), what="VERDICT case, coupled")


def test_the_verdict_case_at_the_gpu_tests_length(emul, rules):
    """2 (S + W) + 7 frames: what tests/test_split_warmup_gpu.py runs -- two seams under the coupled rule."""
    warm = W.emul_rules(rules, W.VERDICT_PD)["coupled"][1]
    fr = W.verdict_frames(W.split_frames(warm))
    o, y, r = _split_errors(emul, W.VERDICT_PD, fr, warm, "coupled, long")
    print("VERDICT case at %d frames: nrms %.3g, worst period %.3g" % (len(fr), r["nrms"], r["worst_window_nrms"]))
    parity.check_oracle(y, o, parity.window_length_of(W.VERDICT_PD), what="VERDICT case at %d frames" % len(fr))


def test_host_model_admits_the_mixed_launchs_up_sampling_voices(emul):
    """tests/test_mixed_split_warmup_gpu.py holds every voice of its launch to the bar under each set's coupled warm-up: the
    voices of the two up-sampling sets pass it by the host model (which has no down-sampling branch)."""
    voices, sets, warm = W.mixed_launch()
    for i, (fr, s) in enumerate(zip(voices, sets)):
        if s == 2:
            continue
        o, y, r = _split_errors(emul, W.MIXED_PDS[s], fr, warm[s], "mixed voice %d" % i)
        parity.check_oracle(y, o, parity.window_length_of(W.MIXED_PDS[s]), what="mixed voice %d (set %d, W = %d)" % (i, s, warm[s]))


def test_the_seeded_population_meets_the_tolerance_under_the_coupled_rule(emul, rules):
    pop = W.population()
    skipped = sum(1 for _, _, fr in pop if fr is None)
    assert skipped <= W.MAX_SKIPPED * len(pop), (skipped, len(pop))
    worst, worst_default, over_default = 0.0, 0.0, 0
    for k, (pd, warm, fr) in enumerate(pop):
        r = W.emul_rules(rules, pd)
        assert r["coupled"][1] == warm, (k, r, warm)
        if fr is None:
            continue
        assert len(fr) == W.split_frames(warm)
        o, y, e = _split_errors(emul, pd, fr, warm, "draw %d" % k)
        _, _, ed = _split_errors(emul, pd, fr, r["default"][1], "draw %d, default" % k)
        worst, worst_default = max(worst, e["nrms"]), max(worst_default, ed["nrms"])
        over_default += ed["nrms"] > RMS_TOL
        assert e["nrms"] <= RMS_TOL, (k, pd, warm, e["nrms"])
        parity.check_oracle(y, o, parity.window_length_of(pd), what="draw %d (W = %d)" % (k, warm))
    print("population: %d draws, %d skipped (W > %d); coupled worst nrms %.3g; default rule: worst %.3g, %d over the tolerance"
          % (len(pop), skipped, W.MAX_POPULATION_WARM, worst, worst_default, over_default))

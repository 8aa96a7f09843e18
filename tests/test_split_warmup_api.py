"""CPU-side checks of the time split's warm-up setting (include/trm_c_api.h: trm_batch_set_split_warmup, trm_split_warm_periods
and their trm_mixed / trm_tube counterparts): the symbols are declared and exported, the enum has its declared values, the raw
entries refuse what has no object behind it, the Python mirrors check their argument before they ask the library, and the
host-only entry trm_split_warm_periods -- no device, no batch object -- gives what the rules' model gives
(tests/test_split_warmup_model.py holds that model against the header and the oracle)."""
import ctypes as C
import os
import re

import pytest

import cases
import golden_io
import split_warmup_common as W
import support
from test_time_split import warm_periods

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["trm_batch_set_split_warmup", "trm_batch_split_warmup", "trm_split_warm_periods", "trm_mixed_set_split_warmup",
       "trm_mixed_split_warmup", "trm_tube_set_split_warmup"]

g = support.product(gpu=False)


def test_new_symbols_are_exported_and_declared(g):
    header = support.assert_exported_and_declared(g, NEW)
    # the rule, the refusals and the statement on streams stand in the comment
    assert "rho_c = (c + sqrt(c^2 + 4 d^2 (1 - c))) / 2" in header
    assert "may lengthen the warm-up and" in header and "never shorten it: TRM_ERANGE" in header
    assert "A stream never splits, so nothing here applies to streams" in header


def test_enum_values_are_as_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    m = re.search(r"enum\s*\{\s*TRM_SPLIT_WARMUP_DEFAULT\s*=\s*(-?\d+)\s*,\s*TRM_SPLIT_WARMUP_COUPLED\s*=\s*(-?\d+)\s*\}", header)
    assert m and [int(x) for x in m.groups()] == [0, -1]
    assert (g._capi.TRM_SPLIT_WARMUP_DEFAULT, g._capi.TRM_SPLIT_WARMUP_COUPLED) == (0, -1)


def test_raw_entries_refuse_a_null_object(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    for v in (0, -1, 45, -2):
        assert L.trm_batch_set_split_warmup(None, v) == E
        assert L.trm_mixed_set_split_warmup(None, v) == E
        assert L.trm_tube_set_split_warmup(None, v) == E
    assert L.trm_batch_split_warmup(None) == 0 and L.trm_mixed_split_warmup(None) == 0
    assert L.trm_split_warm_periods(None, 0) == 0


def test_python_mirrors_check_their_argument_before_they_ask_the_library(g):
    code = g._capi.split_warmup_code
    assert (code("default"), code("coupled"), code(45), code(1)) == (0, -1, 45, 1)
    assert code("coupled", periods_ok=False) == -1
    for bad in ("auto", "COUPLED", None, 0, -1, -3, 2.5, True, [45]):
        with pytest.raises((ValueError, TypeError)):
            code(bad)
    with pytest.raises(ValueError, match="mixed batch"):
        code(45, periods_ok=False)
    assert [g._capi.split_warmup_name(c) for c in (0, -1, 189)] == ["default", "coupled", 189]
    # the classes carry the setter and the property; without an object behind them the bad argument is refused first
    for cls in (g.TRMBatch, g.TRMMixedBatch, g.TRMTubeModel):
        assert callable(getattr(cls, "set_split_warmup")) and isinstance(getattr(cls, "split_warmup"), property), cls
        x = object.__new__(cls)
        x._h = None
        for bad in ("auto", 0, -1, 2.5):
            with pytest.raises(ValueError, match="split warm-up"):
                x.set_split_warmup(bad)
    x = object.__new__(g.TRMMixedBatch)
    x._h = None
    with pytest.raises(ValueError, match="mixed batch"):
        x.set_split_warmup(45)
    # several devices: the host-buffer entries only
    with pytest.raises(NotImplementedError):
        g.TRMMultiBatch.set_split_warmup(object.__new__(g.TRMMultiBatch), "coupled")


def test_host_only_entry_gives_what_the_rules_model_gives(g):
    """No device is asked for: this runs on a host without one."""
    ip = g.TRMInputParameters.from_dict
    sets = [golden_io.load(n)["params_dict"] for n in golden_io.CASE_NAMES] + [W.VERDICT_PD, W.DOWN_PD, W.SHORT_22K_PD]
    sets += [pd for pd, _, _ in W.population(12)]
    for pd in sets:
        cp = W.control_period_of(pd)
        got = {r: g.split_warm_periods(ip(pd), r) for r in ("default", "coupled")}
        assert got == {r: W.rule_periods(pd, cp, r) for r in ("default", "coupled")}, pd
        assert got["default"] == warm_periods(pd, cp) and got["coupled"] >= got["default"] > 0
    monet = cases.monet_default_params(44100.0)
    assert (g.split_warm_periods(ip(monet)), g.split_warm_periods(ip(monet), "coupled")) == (30, 45)
    assert (g.split_warm_periods(ip(W.VERDICT_PD)), g.split_warm_periods(ip(W.VERDICT_PD), "coupled")) == (16, 189)
    # 0: never forgets; parameters the library refuses; a rule it does not know
    L = g.lib()
    assert g.split_warm_periods(ip(dict(monet, lossFactor=0.0)), "coupled") == 0 and g.split_warm_periods(ip(dict(monet, lossFactor=0.0))) == 0
    assert g.split_warm_periods(ip(dict(monet, length=0.0)), "coupled") == 0
    p = ip(monet)
    assert L.trm_split_warm_periods(C.byref(p.c), -2) == 0 and L.trm_split_warm_periods(C.byref(p.c), 45) == 0
    with pytest.raises(ValueError):
        g.split_warm_periods(p, 45)

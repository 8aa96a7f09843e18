"""What the test modules share and tests/conftest.py cannot give them: factories of the fixtures every module used to paste, and
a few helpers.  A fixture takes the name it is assigned to in the module, so scope, name, parameters and parameter ids stay the
module's own:

    g = support.product(gpu=True)
    form = support.kernel_form(["quad", "wide"])
"""
import os

import numpy as np
import pytest

import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "trm_c_api.h")


def product(gpu, after=None):
    """a module-scoped fixture: gnuspeech_amd with its library loaded, on a device where `gpu`; `after()` runs at tear-down"""
    @pytest.fixture(scope="module")
    def fixture():
        import gnuspeech_amd
        L = gnuspeech_amd.lib()
        if gpu:
            assert L.trm_device_count() >= 1
        yield gnuspeech_amd
        if after is not None:
            after()
    return fixture


def kernel_form(forms, autouse=False, note=None):
    """a fixture over `forms`: the kernel form every launch left on TRM_KERNEL_AUTO takes, forced by TRM_TUBE_KERNEL (read when a
    batch or stream is created).  "quad1" is the four-lane form's second instance (one block per pipeline step, the one that lets
    two workgroups share a CU and that batches of more than 16 voices x CUs run): TRM_QUAD_CUS=1 makes every batch take it.
    note: a dict whose "now" names the form for the module's helpers that take no fixture."""
    @pytest.fixture(params=list(forms), autouse=autouse)
    def fixture(request, monkeypatch):
        monkeypatch.setenv("TRM_TUBE_KERNEL", "quad" if request.param == "quad1" else request.param)
        if request.param == "quad1":
            monkeypatch.setenv("TRM_QUAD_CUS", "1")
        else:
            monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
        if note is not None:
            note["now"] = request.param
        return request.param
    return fixture


def no_plan_by_environment():
    """an autouse fixture: no kernel form and no time split forced from the environment, so the test's own settings decide"""
    @pytest.fixture(autouse=True)
    def fixture(monkeypatch):
        monkeypatch.delenv("TRM_TUBE_KERNEL", raising=False)
        monkeypatch.delenv("TRM_QUAD_CUS", raising=False)
        monkeypatch.delenv("TRM_TIME_SPLIT", raising=False)
    return fixture


def sets_of(default_pds):
    """a *_common module's sets(g, pds=its own PDS): the parameter dicts as TRMInputParameters of the package `g`"""
    def sets(g, pds=default_pds):
        return [g.TRMInputParameters.from_dict(p) for p in pds]
    return sets


def layout_of(default_seed, default_sizes, default_gset):
    """a *_common module's layout(seed, sizes, gset), its own constants the defaults: (sets, groups) of the caller's voices, dealt in
    a shuffled order -- sizes[gr] voices in group gr, which runs set gset[gr]"""
    def layout(seed=default_seed, sizes=default_sizes, gset=default_gset):
        groups = np.concatenate([np.full(n, gr, dtype=np.int64) for gr, n in enumerate(sizes)])
        groups = np.random.default_rng(seed).permutation(groups)
        return np.asarray(gset, dtype=np.int64)[groups], groups
    return layout


def input_params(g, **kw):
    """TRMInputParameters of the Monet defaults with `kw` laid over them"""
    return g.TRMInputParameters.from_dict(dict(cases.monet_default_params(), **kw))


def assert_exported_and_declared(g, names):
    """each name is in the binding's export list, declared as a function in include/trm_c_api.h and found in the loaded library;
    returns the header's text for what else the caller looks for in it"""
    header = open(HEADER).read()
    for name in names:
        assert name in g._capi.EXPORTS, name
        assert name + "(" in header, name
        getattr(g.lib(), name)
    return header

"""Oracle against the reference's C tube on random tracks: against what it computed, frozen in
tests/golden/random_tracks_seed<N>.npz (tests/golden/make_golden.py), and against the binary RUN LIVE
where oracle/_ref/tube_ref was built (only where the reference sources are present)."""
import numpy as np
import pytest

import cases
import golden_io
import oracle_lib as O


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_tracks_bit_exact(oracle, tmp_path, seed):
    name = "random_tracks_seed%d" % seed
    pd, fr = cases.random_track_cases((seed,))[name]
    p = oracle.InputParams.from_dict(pd)
    g = golden_io.load(name)
    assert g["params_dict"] == pd and np.array_equal(g["frames"], fr)      # the fixture was made from these very inputs
    refs = [g]
    if O.have_ref():
        refs.append(oracle.run_ref(p, fr, str(tmp_path)))
    o = oracle.synthesize(p, fr, keep_tube=True)
    for r in refs:
        assert o["numberSamples"] == r["numberSamples"]
        assert o["maximumSampleValue"] == r["maximumSampleValue"]
        assert np.array_equal(o["tubeSamples"], r["tubeSamples"])
        assert np.array_equal(o["samples"].astype(np.float32), r["samples_f32"])


# (output rate at the Monet default tube, 19 750 Hz; a frame count that ends on the converter's extra lap; one that does not)
DEEP_RATIOS = [(4000.0, 22, 21), (1600.0, 148, 147), (1000.0, 285, 284), (522.0, 9, 12)]


@pytest.mark.parametrize("rate,lap,plain", DEEP_RATIOS)
def test_deep_down_sampling_live(oracle, tmp_path, rate, lap, plain):
    """The down-sampling converter at 4.9, 12.3, 19.75 and 37.8 tube samples per output -- up to the ratio limit trm_derive sets
    (padSize 493), which rests on the oracle's sample counts there -- against the reference binary run live: identical
    numberSamples with and without the extra lap of the ring (TRMSampleRateConverter.m:160-163), identical tube samples,
    converter output equal after fp32 rounding."""
    if not O.have_ref():
        pytest.skip("oracle/_ref/tube_ref not built (the reference sources are not on this machine)")
    pd = cases.monet_default_params(rate)
    p = oracle.InputParams.from_dict(pd)
    rows = cases.load_gnuspeech_rows()
    for n in (lap, plain):
        fr = rows[:n].copy()
        o = oracle.synthesize(p, fr, keep_tube=True)
        r = oracle.run_ref(p, fr, str(tmp_path))
        d = o["derived"]
        assert (d["padSize"], d["timeRegisterIncrement"], d["phaseIncrement"]) == (r["padSize"], r["timeRegisterIncrement"], r["phaseIncrement"])
        inc = d["timeRegisterIncrement"]
        without = (((n - 1) * d["controlPeriod"] + 2 * d["padSize"]) * 65536 + inc - 1) // inc
        assert (r["numberSamples"] != without) == (n == lap), (rate, n, r["numberSamples"], without)
        assert o["numberSamples"] == r["numberSamples"]
        assert o["maximumSampleValue"] == r["maximumSampleValue"]
        assert np.array_equal(o["tubeSamples"], r["tubeSamples"])
        assert np.array_equal(o["samples"].astype(np.float32), r["samples_f32"])

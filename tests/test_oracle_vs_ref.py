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

"""The down-sampling converter's output count and its ratio limit, without a GPU.

trm_samples_for_frames (src_count_outputs, trm_lane.h: the function the kernels evaluate too) against the oracle's numberSamples
at every launch path's ratios and on both sides of every edge between the paths (tests/downsample_paths_common.py), from 1.01
to 37.9 tube samples per output; and the limit trm_derive sets behind that: the converter's ring takes in 1024 - 2 padSize
samples between two runs, and once that is less than one output's advance (padSize 494 and up) the reference's count leaves
the rule -- at padSize 512 the closed form would divide by zero.  Such parameters are refused (TRM_ERANGE) by every create."""
import numpy as np
import pytest

import cases
import downsample_paths_common as P
import oracle_lib as O
import support

TRM_ERANGE = 10

# (tube length cm, output rate): the path sets, the T1 / T2 edge (48 KB of LDS), the shallowest ratio, the last two pad sizes
# inside the limit at two tube rates
COUNT_SETS = [P.PATH_SETS[k][:2] for k in P.PATH_SETS] + [(17.5, 19550.0), (17.5, 7400.0), (17.5, 7300.0), (17.5, 522.0), (17.5, 521.0),
                                                         (10.0, 916.5)]
COUNT_FRAMES = list(range(1, 61)) + list(range(71, 301, 11))

g = support.product(gpu=False)


def _ip(g, length, rate):
    pd = cases.monet_default_params(rate)
    pd["length"] = length
    return pd, g.TRMInputParameters.from_dict(pd)


def test_path_table_is_what_the_two_rules_give(g):
    """Every set of the path table: the path, taps, tile bytes, row quotient and padSize written there by hand are what
    trm_derive's constants give under launch_downsample's and trm_batch_create's rules -- both sides of each edge included."""
    from gnuspeech_amd import shard
    for name, (length, rate, path, taps, tile, quot, pad) in P.PATH_SETS.items():
        d = shard.derive(_ip(g, length, rate)[1])
        assert P.path_facts(d) == (path, taps, tile, quot) and d["padSize"] == pad, (name, P.path_facts(d), d["padSize"])
        assert d["sampleRate"] == (28500 if length == 12.2 else 19750)
    assert P.PATH_SETS["T2_edge_3700"][4] <= P.DOWN_LDS_MAX < P.PATH_SETS["G1_edge_3650"][4]
    assert P.PATH_SETS["G1_edge_1600"][5] == P.ROW_TAPS_MAX == P.PATH_SETS["G2_edge_1590"][5] - 1
    d = shard.derive(_ip(g, 17.5, 525.0)[1])
    assert P.SRC_RING - 2 * d["padSize"] == 44
    paths = [P.path_facts(shard.derive(_ip(g, 17.5, r)[1])) for r in (7400.0, 7300.0)]
    assert paths[0][0] == "T1" and paths[1][0] == "T2" and paths[0][2] <= 48 * 1024 < paths[1][2], paths


def test_committed_frame_counts_are_what_the_search_finds(g):
    """downsample_paths_common.FRAMES == choose_frames() over trm_samples_for_frames, and every batch has the shape the GPU
    tests rely on: 35 voices, 0 / 1 / 2 frames among them, the longest last but one, the rest at most 130 frames; an
    extra-lap voice beside a neighbour without one and the time tile's edge wherever the count rule offers them."""
    from gnuspeech_amd import shard
    seen_extra = seen_edge = 0
    for name in P.PATH_SETS:
        ip = _ip(g, *P.PATH_SETS[name][:2])[1]
        d = shard.derive(ip)
        count = lambda n: shard.samples_for_frames(ip, n)
        fr = P.FRAMES[name]
        assert fr == P.choose_frames(d, count), name
        assert len(fr) == P.NVOICES == 35 and {0, 1, 2} <= set(fr) and fr[-2] == max(fr) and fr[-1] < fr[-2]
        extra = [n for n in fr if n and count(n) != P.plain_count(d, n)]
        assert sum(n > P.SHORT_MAX for n in fr) <= 5 and max(fr) <= P.LONG_MAX
        if any(count(n) != P.plain_count(d, n) for n in range(3, P.LONG_MAX + 1)):
            assert extra and any(m in fr and m not in extra for n in extra for m in (n - 1, n + 1)), name
            seen_extra += 1
        edge = {count(n) % 64 for n in fr if count(n) >= 63}
        for rem in (63, 0, 1):
            if any(count(n) >= 63 and count(n) % 64 == rem for n in range(3, P.LONG_MAX + 1)):
                assert rem in edge, (name, rem)
                seen_edge += 1
    assert seen_extra >= 6 and seen_edge >= 15          # (4 kHz, 1 kHz and the near-limit set among them)
    for name in ("T2_4k", "G2_1k", "G2_limit_525"):
        ip = _ip(g, *P.PATH_SETS[name][:2])[1]
        d = shard.derive(ip)
        assert any(shard.samples_for_frames(ip, n) != P.plain_count(d, n) for n in P.FRAMES[name] if n), name


@pytest.mark.parametrize("length,rate", COUNT_SETS)
def test_closed_form_count_equals_the_oracle(g, length, rate):
    """trm_samples_for_frames == the oracle's numberSamples, frame counts 1..60 and every 11th up to 300."""
    from gnuspeech_amd import shard
    pd, ip = _ip(g, length, rate)
    d = shard.derive(ip)
    op = O.InputParams.from_dict(pd)
    rc, od = O.derive(op)
    assert rc == 0 and all(od[k] == d[k] for k in ("controlPeriod", "sampleRate", "timeRegisterIncrement", "phaseIncrement", "padSize"))
    assert shard.samples_for_frames(ip, 0) == 0
    frames = np.zeros((COUNT_FRAMES[-1], 16))           # (silence: the count does not depend on the samples)
    laps = 0
    for n in COUNT_FRAMES:
        o = O.synthesize(op, frames[:n])
        got = shard.samples_for_frames(ip, n)
        assert got == o["numberSamples"], "%g cm @ %g Hz (pad %d), %d frames: %d, oracle %d" % (length, rate, d["padSize"], n, got, o["numberSamples"])
        laps += got != P.plain_count(d, n)
    print("%g cm @ %g Hz: %.2f tube samples per output, pad %d, %s; %d of %d frame counts end on the extra lap"
          % (length, rate, d["timeRegisterIncrement"] / 65536.0, d["padSize"], P.path_facts(d)[0], laps, len(COUNT_FRAMES)))


def test_count_sets_span_the_ratios(g):
    from gnuspeech_amd import shard
    ds = sorted(shard.derive(_ip(g, l, r)[1])["timeRegisterIncrement"] / 65536.0 for l, r in COUNT_SETS)
    assert len(ds) >= 12 and ds[0] < 1.011 and ds[-1] > 37.8
    pads = {shard.derive(_ip(g, l, r)[1])["padSize"] for l, r in COUNT_SETS}
    assert {490, 492, 493} <= pads


# output rate at the Monet default tube (19 750 Hz) -> the padSize the reference derives (TRMSampleRateConverter.m:96)
REFUSED = {520.0: 494, 502.5: 511, 501.5: 512, 500.5: 513, 300.0: 856}


@pytest.mark.parametrize("rate,pad", sorted(REFUSED.items()))
def test_ratio_limit_refuses(g, rate, pad):
    """padSize 494 (the first whose ring fill, 36, is under one output's advance, 37.98), 511, 512 (fill 0: the closed form's
    divisor), 513 and 856 (the ring's window wraps over itself): trm_derive returns TRM_ERANGE, trm_samples_for_frames 0."""
    from gnuspeech_amd import shard
    pd, ip = _ip(g, 17.5, rate)
    rc, od = O.derive(O.InputParams.from_dict(pd))
    assert rc == 0 and od["padSize"] == pad                     # (the oracle derives them as the reference does)
    assert (P.SRC_RING - 2 * pad) * 65536 < od["timeRegisterIncrement"]
    with pytest.raises(g.TrmError) as e:
        shard.derive(ip)
    assert e.value.code == TRM_ERANGE
    for n in (1, 2, 20, 300):
        assert shard.samples_for_frames(ip, n) == 0


def test_ratio_limit_is_the_fill_rule_exactly(g):
    """The last pad sizes inside the limit are accepted (493: fill 38 >= 37.91, at two tube rates), and the rule is the one
    inequality: over a sweep of output rates trm_derive refuses exactly where (1024 - 2 pad) 2^16 < timeRegisterIncrement."""
    from gnuspeech_amd import shard
    for length, rate in ((17.5, 521.0), (10.0, 916.5)):
        d = shard.derive(_ip(g, length, rate)[1])
        assert d["padSize"] == 493 and (P.SRC_RING - 2 * 493) * 65536 >= d["timeRegisterIncrement"]
    seen = set()
    for length in (17.5, 10.0):
        for rate in np.arange(200.0, 1200.0, 1.5):
            pd, ip = _ip(g, length, float(rate))
            rc, od = O.derive(O.InputParams.from_dict(pd))
            want_ok = (P.SRC_RING - 2 * od["padSize"]) * 65536 >= od["timeRegisterIncrement"]
            try:
                shard.derive(ip)
                ok = True
            except g.TrmError as e:
                assert e.code == TRM_ERANGE
                ok = False
            assert ok == want_ok, (length, rate, od)
            seen.add(ok)
    assert seen == {True, False}


def test_every_create_names_the_refused_set(g):
    """The limit sits in build_const, so each create path inherits it; the mixed batch and both mixed streams name the set
    (validated before a device is looked for)."""
    ok = g.TRMInputParameters.from_dict(cases.monet_default_params(16000.0))
    bad = _ip(g, 17.5, 501.5)[1]
    for make in (lambda: g.TRMMixedBatch([ok, bad]), lambda: g.TRMMixedStream([ok, bad], [0, 1]),
                 lambda: g.TRMGroupedStream([ok, bad], [0, 1], [0, 1])):
        with pytest.raises(g.TrmError) as e:
            make()
        assert e.value.code == TRM_ERANGE and "parameter set 1" in str(e.value), str(e.value)
    with pytest.raises(g.TrmError) as e:
        g.TRMBatch(bad)
    assert e.value.code == TRM_ERANGE

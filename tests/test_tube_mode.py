"""The mode of a tube launch without a GPU: gnuspeech_amd/csrc/trm_kernels.h states once (tube_mode) which of the seven modes a
launch runs in, from which of four of its tables are set -- seg_periods, mix_map, stream_state, grp_clock --, and launch_tube,
launch_tube_quad and launch_tube_oct switch over that answer.  tests/_emul/tube_mode_table.cc prints the answer for all sixteen
combinations; here it is held against the table below.

Seven combinations are built by the host, one per mode: they are marked, and their rows are what the three launchers picked, each
with a ladder of its own, before the rule was stated once.  No host path builds the other nine: a grp_clock is assigned in one
place (trm_stream_step.cc, step_synthesize), together with stream_state and mix_map, and the time-split paths (trm_capi.cc,
trm_mixed.cc) set seg_periods on launches without a stream_state.  Their rows state where the order of tube_mode's questions
puts them -- segments first, then streams, then the map; a grp_clock counts on a mixed stream alone --, so that a change of that
order shows."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_SHOT, STREAM, SEGMENTS, MIXED, MIXED_STREAM, MIXED_SEGMENTS, GROUP_STREAM = range(7)      # trm_kernels.h: kMode*
HOST = True

# (seg_periods, mix_map, stream_state, grp_clock) set -> (mode, a host path builds the combination)
TABLE = {
    (0, 0, 0, 0): (ONE_SHOT, HOST),
    (1, 0, 0, 0): (SEGMENTS, HOST),
    (0, 1, 0, 0): (MIXED, HOST),
    (1, 1, 0, 0): (MIXED_SEGMENTS, HOST),
    (0, 0, 1, 0): (STREAM, HOST),
    (1, 0, 1, 0): (SEGMENTS, False),
    (0, 1, 1, 0): (MIXED_STREAM, HOST),
    (1, 1, 1, 0): (MIXED_SEGMENTS, False),
    (0, 0, 0, 1): (ONE_SHOT, False),
    (1, 0, 0, 1): (SEGMENTS, False),
    (0, 1, 0, 1): (MIXED, False),
    (1, 1, 0, 1): (MIXED_SEGMENTS, False),
    (0, 0, 1, 1): (STREAM, False),
    (1, 0, 1, 1): (SEGMENTS, False),
    (0, 1, 1, 1): (GROUP_STREAM, HOST),
    (1, 1, 1, 1): (MIXED_SEGMENTS, False),
}


def test_tube_mode_table(tmp_path):
    assert len(TABLE) == 16
    built = sorted(mode for mode, host in TABLE.values() if host)
    assert built == list(range(7)), "the host builds one combination per mode"
    exe = str(tmp_path / "tube_mode_table")
    # (host code alone: the program holds no kernel)
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-fno-exceptions", "--offload-host-only",
                           os.path.join(ROOT, "tests", "_emul", "tube_mode_table.cc"), "-o", exe])
    got = [int(w) for w in subprocess.check_output([exe], text=True).split()]
    assert len(got) == 16
    for m, mode in enumerate(got):
        key = (m & 1, m >> 1 & 1, m >> 2 & 1, m >> 3 & 1)
        print(key, "->", mode, "(host)" if TABLE[key][1] else "")
        assert mode == TABLE[key][0], (key, mode, TABLE[key])

"""The down-sampling converter's four launch paths: the parameter sets that reach each of them and both sides of
every edge between them, and the ragged batch each set is run with.  Shared by tests/test_downsample_paths_gpu.py (the paths
against the oracle), tests/test_downsample_counts.py (the closed-form output count, the ratio limit) and
tests/test_downsample_model.py (the host model of the two kernels' product orders).

    T1  tile <= 48 KB of LDS                 trm_downsample_rows_kernel
    T2  48 KB < tile <= 96 KB                the same kernel under a raised dynamic-LDS allowance
    G1  rows built, tile over 96 KB          trm_downsample_kernel (the generic walk over the fine table)
    G2  more than 160 taps a wing: no rows   the generic walk, rows == nullptr

Every number of PATH_SETS is hand arithmetic from launch_downsample's rule (trm_kernels.hip: down_tile_lds, kDownLdsMax) and
trm_batch_create's row rule (trm_capi.cc: kSrcFineLen / phaseIncrement <= 160); path_facts() recomputes them from trm_derive
and the tests compare, so a set that drifts to another path says so."""
import numpy as np

import cases

SRC_FINE_LEN = 13 * 256 * 256        # entries of the fine table (trm_setup.cc: build_src_fine)
SRC_RING = 1024                      # TRMRingBuffer.h BUFFER_SIZE
DOWN_COLS, DOWN_VOICES = 64, 32      # the tiled kernel's tile: outputs x voices (trm_kernels.hip)
DOWN_LDS_MAX = 96 * 1024
ROW_TAPS_MAX = 160

# name: (tube length cm, output rate Hz, path, taps a wing, tile bytes, kSrcFineLen / phaseIncrement, padSize)
PATH_SETS = {
    "T1_16k":       (17.5, 16000.0, "T1", 17, 23424, 16, 17),
    "T2_8k_12cm":   (12.2, 8000.0, "T2", 47, 65280, 46, 47),
    "T2_4k":        (17.5, 4000.0, "T2", 65, 90240, 64, 65),
    "T2_edge_3700": (17.5, 3700.0, "T2", 70, 97280, 69, 70),
    "G1_edge_3650": (17.5, 3650.0, "G1", 71, 98560, 70, 71),
    "G1_3k":        (17.5, 3000.0, "G1", 86, 119552, 85, 86),
    "G1_edge_1600": (17.5, 1600.0, "G1", 161, 223616, 160, 161),
    "G2_edge_1590": (17.5, 1590.0, "G2", 162, 225024, 161, 162),
    "G2_1k":        (17.5, 1000.0, "G2", 257, 357120, 256, 257),
    "G2_limit_525": (17.5, 525.0, "G2", 490, 680192, 489, 490),
}
GPU_SETS = [k for k in PATH_SETS if k != "T1_16k"]          # (T1 is tests/test_gpu_parity.py's)


def params_of(name):
    length, rate = PATH_SETS[name][:2]
    pd = cases.monet_default_params(rate)
    pd["length"] = length
    return pd


def path_facts(d):
    """(path, taps a wing, tile bytes, quotient) of a trm_derived dict, by the library's two rules."""
    ph, inc = d["phaseIncrement"], d["timeRegisterIncrement"]
    taps = (SRC_FINE_LEN + ph - 1) // ph                       # build_down_rows: lmax = rmax
    T = 2 * taps
    xlen = ((DOWN_COLS - 1) * inc >> 16) + 2 + T
    tile = (DOWN_COLS * (T | 1) + DOWN_VOICES * xlen) * 4      # down_tile_lds
    quot = SRC_FINE_LEN // ph
    path = "G2" if quot > ROW_TAPS_MAX else "G1" if tile > DOWN_LDS_MAX else "T2" if tile > 48 * 1024 else "T1"
    return path, taps, tile, quot


def plain_count(d, nframes):
    """Outputs of a voice without the reference's extra lap: ceil((ntube + 2 pad) 2^16 / inc)."""
    if nframes == 0:
        return 0
    inc = d["timeRegisterIncrement"]
    return (((nframes - 1) * d["controlPeriod"] + 2 * d["padSize"]) * 65536 + inc - 1) // inc


# ---------------------------------------------------------------- the ragged batch of a set
NVOICES = 35                # the 32-voice tile and 3 over
SHORT_MAX, LONG_MAX = 130, 400


def choose_frames(d, count):
    """The 35 frame counts a set is run with, from the count rule alone (count(n) = trm_samples_for_frames): voices of 0, 1 and
    2 frames; the first frame count <= 400 that ends on the reference's extra lap beside a neighbour that does not; the first
    counts (<= 130 frames if there are any, else <= 400) whose outputs are 64k-1, 64k and 64k+1, the time tile's edge; the rest
    spread over 3..130 frames; the longest voice last but one."""
    picked = [0, 1, 2]
    extra = [n for n in range(3, LONG_MAX + 1) if count(n) != plain_count(d, n)]
    for n in extra:
        nb = [m for m in (n - 1, n + 1) if 3 <= m <= LONG_MAX and m not in extra]
        if nb:
            picked += [n, nb[0]]
            break
    for rem in (63, 0, 1):
        hit = [n for n in range(3, LONG_MAX + 1) if count(n) >= 63 and count(n) % DOWN_COLS == rem]
        short = [n for n in hit if n <= SHORT_MAX]
        if short or hit:
            picked.append((short or hit)[0])
    fill = NVOICES - len(picked)
    picked += [3 + (i * (SHORT_MAX - 3)) // (fill - 1) for i in range(fill)]
    longest = max(range(NVOICES), key=lambda i: picked[i])
    picked.append(picked.pop(longest))                         # the longest to the end ...
    picked[-1], picked[-2] = picked[-2], picked[-1]            # ... then last but one
    return picked


# choose_frames() of every set, as found on the CPU (tests/test_downsample_counts.py keeps the two in step)
FRAMES = {
    "T1_16k": [0, 1, 2, 3, 7, 11, 15, 19, 23, 27, 31, 35, 39, 43, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 89, 93, 97, 101, 105, 109, 113, 117, 121, 130, 125],
    "T2_8k_12cm": [0, 1, 2, 3, 7, 11, 15, 19, 23, 27, 31, 35, 39, 43, 48, 52, 56, 60, 64, 68, 72, 76, 80, 84, 89, 93, 97, 101, 105, 109, 113, 117, 121, 130, 125],
    "T2_4k": [0, 1, 2, 22, 21, 3, 7, 11, 16, 20, 24, 29, 33, 38, 42, 46, 51, 55, 59, 64, 68, 73, 77, 81, 86, 90, 94, 99, 103, 108, 112, 116, 121, 130, 125],
    "T2_edge_3700": [0, 1, 2, 44, 43, 51, 77, 116, 3, 7, 12, 17, 22, 27, 32, 37, 42, 46, 51, 56, 61, 66, 71, 76, 81, 86, 90, 95, 100, 105, 110, 115, 120, 130, 125],
    "G1_edge_3650": [0, 1, 2, 188, 21, 43, 8, 3, 7, 12, 17, 22, 27, 32, 37, 42, 46, 51, 56, 61, 66, 71, 76, 81, 86, 90, 95, 100, 105, 110, 115, 120, 125, 189, 130],
    "G1_3k": [0, 1, 2, 4, 3, 7, 11, 15, 19, 24, 28, 32, 36, 41, 45, 49, 53, 58, 62, 66, 70, 74, 79, 83, 87, 91, 96, 100, 104, 108, 113, 117, 121, 130, 125],
    "G1_edge_1600": [0, 1, 2, 147, 7, 3, 7, 12, 16, 21, 25, 30, 34, 39, 43, 48, 52, 57, 61, 66, 71, 75, 80, 84, 89, 93, 98, 102, 107, 111, 116, 120, 125, 148, 130],
    "G2_edge_1590": [0, 1, 2, 182, 47, 17, 7, 3, 7, 12, 17, 22, 27, 32, 37, 42, 46, 51, 56, 61, 66, 71, 76, 81, 86, 90, 95, 100, 105, 110, 115, 120, 125, 183, 130],
    "G2_1k": [0, 1, 2, 284, 10, 3, 7, 12, 16, 21, 25, 30, 34, 39, 43, 48, 52, 57, 61, 66, 71, 75, 80, 84, 89, 93, 98, 102, 107, 111, 116, 120, 125, 285, 130],
    "G2_limit_525": [0, 1, 2, 6, 5, 36, 6, 98, 3, 7, 12, 17, 22, 27, 32, 37, 42, 46, 51, 56, 61, 66, 71, 76, 81, 86, 90, 95, 100, 105, 110, 115, 120, 130, 125],
}


def voices_of(name):
    """The set's batch: voice i = FRAMES[name][i] frames of gnuspeech.input's rows, read cyclically from row 7 i."""
    rows = cases.load_gnuspeech_rows()
    out = []
    for i, n in enumerate(FRAMES[name]):
        idx = (7 * i + np.arange(n)) % len(rows)
        out.append(rows[idx].copy() if n else np.zeros((0, 16)))
    return out

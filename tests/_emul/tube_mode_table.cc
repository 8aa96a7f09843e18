// tube_mode_table.cc -- TEST INFRASTRUCTURE.  A stand-alone program over gnuspeech_amd/csrc/trm_kernels.h alone
// (tests/test_tube_mode.py): for each of the sixteen combinations of the four tables a tube launch's mode is read from -- bit 0
// seg_periods, bit 1 mix_map, bit 2 stream_state, bit 3 grp_clock, set or not -- it prints what tube_mode answers.  Nothing is
// dereferenced; it calls nothing of the HIP runtime and is never part of libtrm_hip.so.
#include <stdio.h>
#include "../../gnuspeech_amd/csrc/trm_kernels.h"

int main()
{
    static float state[1];
    static const uint4 map[1] = {};
    for (int m = 0; m < 16; m++) {
        trm::TubeArgs a{};
        if (m & 1) a.seg_periods = 7;
        if (m & 2) a.mix_map = map;
        if (m & 4) a.stream_state = state;
        if (m & 8) a.grp_clock = (decltype(a.grp_clock))map;
        printf("%d\n", trm::tube_mode(a));
    }
    return 0;
}

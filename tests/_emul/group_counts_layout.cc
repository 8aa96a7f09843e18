// group_counts_layout.cc -- TEST INFRASTRUCTURE.  A stand-alone program over gnuspeech_amd/csrc/trm_stream_engine.h alone
// (tests/test_group_counts_api.py): for every combination of the stretches a stream may have made room for, it prints the words
// step_words_room gives the step's tables without and with the counts stretch, and where step_layout at its maxima puts that
// stretch and the end.  It calls nothing of the HIP runtime and is never part of libtrm_hip.so.
#include <stdio.h>
#include "../../gnuspeech_amd/csrc/trm_stream_engine.h"

int main()
{
    trm_stream_engine *s = new trm_stream_engine;          // (never destroyed: the destructors belong to the library's units)
    s->gbegin = {0, 3, 70, 71};
    s->mapEntries = 5; s->nvoices = 71; s->downBlocks = 4;
    for (int m = 0; m < 4; m++) {
        const bool down = m & 1, gain = m & 2;
        const StepLayout l = step_layout(5, 3, 71, true, 5, down ? 3 : 0, down ? 4 : 0, gain ? 5 : 0, true);
        printf("%zu %zu %zu %zu\n", step_words_room(s, down, gain, false), step_words_room(s, down, gain, true), l.counts, l.words);
    }
    return 0;
}

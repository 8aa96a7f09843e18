// trm_tracks_mixed.hip -- the mixed-parameter instance of trm_tracks.hip's control-track kernel: the same source compiled again
// under a name of its own, trm_tracks_mixed_kernel, with one trm_intonation per utterance (trm_kernels.h: MixedTrackArgs).
#define TRM_TRACKS_MIXED_TU
#include "trm_tracks.hip"

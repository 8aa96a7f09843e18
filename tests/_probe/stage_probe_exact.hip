// stage_probe_exact.hip -- TEST INFRASTRUCTURE.  Probe 10's kernels once more, in an object built without the compiler's own
// a * b + c fusion (the csrc Makefile's PROBELANEFLAGS, as the lane-form probes are built): tube_step<TubeConst, true> with
// the throat section outside equals tube_step<Const> bit for bit for the operations as the header writes them, and that is
// what this object runs.  Probes 16 and 17 (the lane forms' packed dot products against the written-out forms, bit for bit)
// are built here once more for the same reason.  Part of tests/_probe/libtrm_probe.so; never linked into libtrm_hip.so.
#include "stage_probe_dev.h"

using namespace trm_probe;

extern "C" int trm_probe_step_exact(const trm_input_params *p, int variant, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    return launch_step<1>(p, variant, state, ctl, exc, n, out);
}

extern "C" int trm_probe_lane_fir_exact(const trm_input_params *p, int ahead, const float *seq, int nseq, int steps, float *out)
{
    return launch_lane_fir<1>(p, ahead, seq, nseq, steps, out);
}

extern "C" int trm_probe_cvt_exact(const float *rings, int nrings, const float *rows, const uint32_t *items, int n, float *out)
{
    return launch_cvt<1>(rings, nrings, rows, items, n, out);
}

// stage_probe_exact.hip -- TEST INFRASTRUCTURE.  Probe 10's kernels once more, in an object built without the compiler's own
// a * b + c fusion (the csrc Makefile's PROBELANEFLAGS, as the lane-form probes are built): tube_step<TubeConst, true> with
// the throat section outside equals tube_step<Const> bit for bit for the operations as the header writes them, and that is
// what this object runs.  Part of tests/_probe/libtrm_probe.so; never linked into libtrm_hip.so.
#include "stage_probe_dev.h"

using namespace trm_probe;

extern "C" int trm_probe_step_exact(const trm_input_params *p, int variant, const float *state, const float *ctl, const float *exc, int n, float *out)
{
    return launch_step<1>(p, variant, state, ctl, exc, n, out);
}

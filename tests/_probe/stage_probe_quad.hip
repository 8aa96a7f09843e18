// stage_probe_quad.hip -- TEST INFRASTRUCTURE.  tube_quad_step / tube_quad_core with the real DPP moves against tube_step
// in the same kernel (stage_probe.h, probe 7).  One wave per block, lanes as trm_quad.hip lays them: part = (lane >> 2) & 3,
// voice = (lane >> 4) * 4 + (lane & 3): 16 voices per wave.  Built with the product's QUADFLAGS.
#include "stage_probe_dev.h"

using namespace trm_probe;

__global__ void __launch_bounds__(64) k_quad(Const C, int nwaves, unsigned seed, int poisonOdd, int32_t *bad)
{
    if ((int)blockIdx.x >= nwaves) return;          // (wave-uniform: no lane of a running wave is missing)
    const int lane = threadIdx.x;
    const int part = (lane >> 2) & 3, vq = (lane >> 4) * 4 + (lane & 3);
    const uint32_t voice = blockIdx.x * 16u + (uint32_t)vq;
    bad[blockIdx.x * 64 + lane] = probe_quad_voice<float>(C, voice_seed(seed, voice), poisonOdd && (voice & 1u), part);
}

extern "C" int trm_probe_quad(const trm_input_params *p, int nwaves, unsigned seed, int poison_odd, int32_t *bad)
{
    Const C;
    trm_derived d;
    if (!p || build_const(*p, C, d) || nwaves <= 0 || nwaves > kMaxItems / 64) return (int)hipErrorInvalidValue;
    DevBufs B;
    int32_t *dBad;
    hipError_t e = B.get(&dBad, (size_t)nwaves * 64);
    if (e == hipSuccess) {
        k_quad<<<(unsigned)nwaves, 64>>>(C, nwaves, seed, poison_odd, dBad);
        e = finish(bad, dBad, (size_t)nwaves * 64);
    }
    return result(e, B);
}

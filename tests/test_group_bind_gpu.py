"""Closed groups change their voice type, sets are replaced: on the GPU (include/trm_c_api.h: trm_mixed_stream_group_bind,
trm_mixed_stream_set_params).  Five sets -- 17.5 cm at 44.1 kHz mono; 15 cm at 16 kHz, which down-samples; 16 cm, sine, no
modulation, stereo at balance 0.3; one without voices at create; a spare one whose parameters are replaced -- and groups of 1, 3,
17, 70 and 2 voices run ONE fixed schedule (tests/group_bind_common.py) of utterances of 32 to 41 frames in steps of 7 and 25
frames, in which a group is bound from an up-sampling set to the down-sampling one and runs again, another the other way, the 70
voices to the stereo set and read through step_int16, the 17 to the set that was empty at create, one with its event lists
waiting, one to the spare set after its parameters were replaced, while group 4 stays mid-utterance across all of it.

Every voice is held, step by step, against a TRMStream of the set bound when its utterance opened, with the group's voices:
samples, counts and maxima bit for bit, in both kernel forms and both loop orders; the int16 rows against
trm_batch_scale_to_int16_device of a TRMBatch of that set over the reference's samples under the same level.  No kernel changed
for this: what is tested is that a bind leaves every table a kernel reads current."""
import ctypes as C

import numpy as np
import pytest

import group_bind_common as B
import support

pytestmark = pytest.mark.gpu

_BATCHES = {}
g = support.product(gpu=True, after=lambda: (B._REF.clear(), _BATCHES.clear()))
form = support.kernel_form(["quad", "wide"])


def batch_scaler(g):
    """trm_batch_scale_to_int16_device of a TRMBatch of the set over one voice's fp32 samples with d_max_sample = level
    (as tests/test_group_int16_gpu.py holds the int16 steps)"""
    import torch
    dev = torch.device("cuda", 0)

    def scale(pd, x, level, wav):
        key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in pd.items()))
        if key not in _BATCHES:
            _BATCHES[key] = g.TRMBatch(g.TRMInputParameters.from_dict(pd), device=0)
        b = _BATCHES[key]
        ch = 2 if pd["channels"] == 2 else 1
        d_x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
        off = torch.zeros(1, dtype=torch.int64, device=dev)
        n = torch.tensor([x.size], dtype=torch.int32, device=dev)
        mxs = torch.tensor([level], dtype=torch.float32, device=dev)
        out = torch.zeros(x.size * ch, dtype=torch.int16, device=dev)
        g._capi.check(g.lib().trm_batch_scale_to_int16_device(b._h, 1, d_x.data_ptr(), off.data_ptr(), n.data_ptr(), mxs.data_ptr(), out.data_ptr(),
                                                              int(wav), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy()
    return scale


def test_schedule_contains_every_event():
    ev, lengths = B.events()
    assert ev == B.EVENTS
    assert lengths and all(20 <= n <= 45 and n % 7 and n % 25 for n in lengths), lengths
    assert B.GROUP_SIZE == [1, 3, 17, 70, 2] and {st["n"] for st in B.SCHEDULE} == {0, 7, 25}


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_bit_for_bit_against_a_stream_of_the_set_bound_at_the_time(g, form, mode):
    """the whole schedule; set_of, channels and samples_for are asked after each bind (group_bind_common.run_schedule)"""
    sounding, compared16 = B.run_schedule(g, form, mode, scaler=batch_scaler(g), wav=(mode == "tract"))
    assert sounding >= 20 and compared16 > 10000


def test_refusals_on_the_device(g, form):
    """every refusal, between steps that a twin takes without them: the same bits, so the stream was left as it was"""
    B.check_refusals(g, form)

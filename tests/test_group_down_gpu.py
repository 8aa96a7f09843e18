"""The down-sampling groups of a grouped stream converted in one launch, on the GPU (include/trm_c_api.h:
trm_mixed_stream_set_group_convert; the kernels of gnuspeech_amd/csrc/trm_grp_down.hip).  Four sets -- 17.5 cm at 16 kHz, at 8 kHz
(the wide converter: 66 taps), 15 cm at 22.05 kHz (a ratio just above 1) and a stereo up-sampling
set that rides along -- seven groups of 33, 1, 9, 2, 3, 2 and 1 voices, steps of 7 and 25 frames, staggered starts, a group that
runs from event lists, a second utterance, steps of flushes alone (tests/group_down_common.py).

THE RULE: every step's samples, counts and maxima under "one_launch" are bit for bit those of a twin stepped under "per_group" --
the parent's code -- and those of a TRMStream per group; toggling the path with every step, mid-utterance, changes no sample;
int16 steps are byte-equal with `clipped`; the device entries return what the host entries return and write nothing behind a
row's values; binds between up- and down-sampling sets and a replaced down-sampling set behave alike in both paths."""
import numpy as np
import pytest

import group_bind_common as B
import group_down_common as D
import group_events_common as EV
import support

pytestmark = pytest.mark.gpu
P, F, I, R = D.P, D.F, D.I, D.R

g = support.product(gpu=True, after=B._REF.clear)
form = support.kernel_form(["quad", "wide"])


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_one_launch_is_the_per_group_path_and_a_stream_per_group(g, form, mode):
    sounding, bases, _, _ = D.run_modes(g, form, mode, D.every)
    print("group-steps that sounded: %d; k_base per step: %s" % (sounding, bases))
    assert sounding >= 25
    assert mode == "tract" or D.bases_differ(bases), bases


@pytest.mark.parametrize("mode", ["framework", "tract"])
def test_the_path_toggled_every_step_changes_no_sample(g, form, mode):
    sounding, _, _, _ = D.run_modes(g, form, mode, D.toggled)
    assert sounding >= 25


@pytest.mark.parametrize("wav", [False, True])
def test_int16_steps_are_byte_equal_with_their_clip_counts(g, form, wav):
    _, _, clipped, unsat = D.run_modes(g, form, "framework", D.every, reference=False, int16=True, wav=wav)
    print("clipped %d, not saturated %d" % (clipped, unsat))
    assert clipped > 0 and unsat > 0


def test_binds_and_a_replaced_set_agree_between_the_paths(g, form):
    assert D.run_bind_and_replace(g, form) == 10


FILL, FILL16 = 7.0, 0x7B7B


def test_device_entries_return_the_host_entries_bits_and_leave_the_rest_untouched(g, form):
    """Both streams in one launch: `a` through step_device / step_device_int16 on torch tensors in grouped order, rows wider than
    any count (an odd int16 pitch) and filled with a pattern, `b` through the host entries.  fp32 steps first over the whole
    schedule, which also yields the levels of the int16 pass: 0.7 x each group's maximum in the step, so that values clip."""
    import torch
    dev = torch.device("cuda", 0)
    levels_of = []
    for int16 in (False, True):
        a, groups = D.new_stream(g, convert="one_launch")
        b, _ = D.new_stream(g, convert="one_launch")
        assert a.kernel == form
        V = groups.size
        fr = D.frames_of(V)
        lists, _ = B.run_lists(g, D.GROUP_SIZE[D.RUN_GROUP], D.RUN_F, seed=8)
        a.set_events(D.RUN_GROUP, lists)
        b.set_events(D.RUN_GROUP, lists)
        at = clipped = 0
        for i, st in enumerate(D.SCHEDULE):
            n, acts = st["n"], st["acts"]
            frames = fr[:, at:at + n] if any(x == P for x in acts) else None
            d_f = torch.from_numpy(np.ascontiguousarray(frames[a.order])).to(dev) if frames is not None else None
            mx = torch.full((V,), -1.0, dtype=torch.float32, device=dev)
            if int16:
                rb = b.step_int16(acts, frames, nframes=n, levels=levels_of[i])
                pitch = (rb[0].shape[1] + 2) | 1
                out = torch.full((V, pitch), FILL16, dtype=torch.int16, device=dev)
                cl = torch.full((V,), 77, dtype=torch.int32, device=dev)
                _, nv = a.step_device_int16(acts, d_f, out=out, max_out=mx, clipped=cl, device=dev, nframes=n, levels=levels_of[i])
                torch.cuda.synchronize(dev)
                assert np.array_equal(cl.cpu().numpy().astype(np.uint32)[a.inverse], rb[3]), i
                clipped += int(rb[3].sum())
            else:
                rb = b.step(acts, frames, nframes=n)
                out = torch.full((V, rb[0].shape[1] + 5), FILL, dtype=torch.float32, device=dev)
                _, nv = a.step_device(acts, d_f, out=out, max_out=mx, device=dev, nframes=n)
                torch.cuda.synchronize(dev)
                levels_of.append({gr: float(np.float32(0.7 * max(float(rb[2][groups == gr].max()), 1e-4))) for gr in range(D.G)})
            o = out.cpu().numpy()
            assert np.array_equal(nv[a.inverse], rb[1]) and EV.eq(mx.cpu().numpy()[a.inverse], rb[2]), i
            for j, v in enumerate(a.order):
                assert o[j, :nv[j]].tobytes() == rb[0][v, :nv[j]].tobytes(), (int16, i, v)
                assert np.all(o[j, nv[j]:] == (FILL16 if int16 else FILL)), (int16, i, v)
            at += n
        assert not any(a.is_open(gr) for gr in range(D.G))
        assert not int16 or clipped > 0

"""CPU-side check of the four-lane time split of mixed-parameter batches (include/trm_c_api.h: trm_mixed_set_kernel(QUAD) with
trm_mixed_set_time_split): the mixed segment instance of the four-lane kernel is in the library under a name of its own and
within its register budget."""
import kernel_manifest
import kernel_notes

KERNEL = "_ZN3trm18trm_mixqseg_kernelILb1ELi2ELb1ELb1EEEvNS_5ConstENS_8TubeArgsE"     # trm_mixqseg_kernel<true, 2, true, true>


def test_four_lane_mixed_segment_instance_is_built_under_its_own_name_within_budget():
    """Exactly one kernel of the name (a line of tests/kernel_manifest.py); no scratch, no spills, at most 128 VGPRs."""
    kernel_manifest.check(kernel_notes.read_kernels(), KERNEL)
    assert kernel_manifest.named("trm_mixqseg_kernel") == [KERNEL]

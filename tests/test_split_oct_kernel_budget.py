"""The eight-lane segment instance in the built libtrm_hip.so (gnuspeech_amd/csrc/trm_oct_seg.hip: trm_octseg_kernel), read as
tests/test_capi_exports.py reads every kernel: there is exactly one, it stays within 128 VGPRs -- four waves per SIMD, which with
OctLds (61 KB) puts two workgroups on a CU -- and has no private segment and no spills."""
import kernel_manifest
import kernel_notes

KERNEL = "_ZN3trm17trm_octseg_kernelILb0ELb1EEEvNS_5ConstENS_8TubeArgsE"          # trm_octseg_kernel<false, true>


def test_the_octseg_kernel_is_one_symbol_within_its_register_budget():
    assert kernel_manifest.named("trm_octseg_kernel") == [KERNEL]
    assert kernel_manifest.KERNELS[KERNEL] == 0                                     # (one dynamically sized array: trm_oct.hip, OctLds)
    kernel_manifest.check(kernel_notes.read_kernels(), KERNEL)

"""The kernels of libtrm_hip.so, by exact mangled name: tests/test_capi_exports.py holds the library to this table (these names, each
built once, none with scratch or spills, all within kernel_notes.VGPR_BUDGET), and the per-feature tests look their own kernels
up in it.  A new kernel is one line here.  The value is the kernel's static LDS in bytes where a test pins it, else None."""

KERNELS = {
    # the tube kernels, one voice per lane (trm_kernels.hip): one-shot, stream, time-split segment
    "_ZN3trm15trm_tube_kernelILi0EEEvNS_5ConstENS_8TubeArgsE": None,                        # trm_tube_kernel<0>
    "_ZN3trm15trm_tube_kernelILi1EEEvNS_5ConstENS_8TubeArgsE": None,                        # trm_tube_kernel<1>
    "_ZN3trm15trm_tube_kernelILi2EEEvNS_5ConstENS_8TubeArgsE": None,                        # trm_tube_kernel<2>
    # ... four lanes per voice (trm_quad.hip), eight lanes per voice (trm_oct.hip)
    "_ZN3trm17trm_tube_kernel_qILb0ELi1ELb0ELb0EEEvNS_5ConstENS_8TubeArgsE": None,          # trm_tube_kernel_q<false, 1, false, false>
    "_ZN3trm17trm_tube_kernel_qILb0ELi2ELb0ELb0EEEvNS_5ConstENS_8TubeArgsE": None,          # trm_tube_kernel_q<false, 2, false, false>
    "_ZN3trm17trm_tube_kernel_qILb1ELi2ELb0ELb0EEEvNS_5ConstENS_8TubeArgsE": None,          # trm_tube_kernel_q<true, 2, false, false>
    "_ZN3trm17trm_tube_kernel_qILb1ELi2ELb1ELb0EEEvNS_5ConstENS_8TubeArgsE": None,          # trm_tube_kernel_q<true, 2, true, false>
    "_ZN3trm17trm_tube_kernel_oILb0ELb0EEEvNS_5ConstENS_8TubeArgsE": None,                  # trm_tube_kernel_o<false, false>
    "_ZN3trm17trm_octseg_kernelILb0ELb1EEEvNS_5ConstENS_8TubeArgsE": 0,                     # trm_octseg_kernel<false, true> (its one array is dynamic)
    # their mixed-parameter instances: one-shot, stream, time-split segments, grouped streams
    "_ZN3trm14trm_mix_kernelILi3EEEvNS_5ConstENS_8TubeArgsE": None,                         # trm_mix_kernel<3>
    "_ZN3trm14trm_mix_kernelILi4EEEvNS_5ConstENS_8TubeArgsE": None,                         # trm_mix_kernel<4>
    "_ZN3trm16trm_mix_kernel_qILb0ELi1ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE": None,           # trm_mix_kernel_q<false, 1, false, true>
    "_ZN3trm16trm_mix_kernel_qILb0ELi2ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE": None,           # trm_mix_kernel_q<false, 2, false, true>
    "_ZN3trm16trm_mix_kernel_qILb1ELi2ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE": None,           # trm_mix_kernel_q<true, 2, false, true>
    "_ZN3trm16trm_mix_kernel_oILb1ELb0EEEvNS_5ConstENS_8TubeArgsE": None,                   # trm_mix_kernel_o<true, false>
    "_ZN3trm17trm_mixseg_kernelILi5EEEvNS_5ConstENS_8TubeArgsE": None,                      # trm_mixseg_kernel<5>
    "_ZN3trm18trm_mixqseg_kernelILb1ELi2ELb1ELb1EEEvNS_5ConstENS_8TubeArgsE": None,         # trm_mixqseg_kernel<true, 2, true, true>
    "_ZN3trm20trm_grpstream_kernelILi6EEEvNS_5ConstENS_8TubeArgsE": None,                   # trm_grpstream_kernel<6>
    "_ZN3trm22trm_grpstream_kernel_qILb1ELi2ELb0ELb1EEEvNS_5ConstENS_8TubeArgsE": None,     # trm_grpstream_kernel_q<true, 2, false, true>
    # control tracks from event lists
    "_ZN3trm17trm_tracks_kernelENS_9TrackArgsE": None,                                      # trm_tracks_kernel(TrackArgs)
    "_ZN3trm21trm_tracks_run_kernelENS_12TrackRunArgsE": None,                              # trm_tracks_run_kernel(TrackRunArgs)
    "_ZN3trm23trm_tracks_mixed_kernelENS_14MixedTrackArgsE": None,                          # trm_tracks_mixed_kernel(MixedTrackArgs)
    # the time split's pre-pass
    "_ZN3trm23trm_phase_period_kernelENS_5ConstENS_9PhaseArgsE": None,                      # trm_phase_period_kernel(Const, PhaseArgs)
    "_ZN3trm24trm_phase_segment_kernelENS_5ConstENS_9PhaseArgsE": None,                     # trm_phase_segment_kernel(Const, PhaseArgs)
    "_ZN3trm18trm_seg_map_kernelENS_9PhaseArgsE": None,                                     # trm_seg_map_kernel(PhaseArgs)
    "_ZN3trm21trm_seg_blocks_kernelENS_9PhaseArgsE": None,                                  # trm_seg_blocks_kernel(PhaseArgs)
    "_ZN3trm22trm_split_clear_kernelEPfjPj": None,                                          # trm_split_clear_kernel(float*, unsigned, unsigned*)
    # sample-rate conversion
    "_ZN3trm21trm_down_count_kernelENS_5ConstENS_8DownArgsE": None,                         # trm_down_count_kernel(Const, DownArgs)
    "_ZN3trm21trm_downsample_kernelENS_5ConstENS_8DownArgsE": None,                         # trm_downsample_kernel(Const, DownArgs)
    "_ZN3trm26trm_downsample_rows_kernelENS_5ConstENS_8DownArgsEj": None,                   # trm_downsample_rows_kernel(Const, DownArgs, unsigned)
    "_ZN3trm22trm_grp_hist_in_kernelENS_11GrpDownArgsE": None,                              # trm_grp_hist_in_kernel(GrpDownArgs)
    "_ZN3trm22trm_grp_convert_kernelENS_11GrpDownArgsE": None,                              # trm_grp_convert_kernel(GrpDownArgs)
    # output: gain, int16 PCM, sound-file images, noise
    "_ZN3trm15trm_gain_kernelEPfmjjS0_f": None,                                             # trm_gain_kernel(float*, unsigned long, unsigned, unsigned, float*, float)
    "_ZN3trm16trm_int16_kernelENS_9ScaleArgsE": None,                                       # trm_int16_kernel(ScaleArgs)
    "_ZN3trm21trm_file_image_kernelENS_8FileArgsE": None,                                   # trm_file_image_kernel(FileArgs)
    "_ZN3trm22trm_mixed_int16_kernelENS_10MixOutArgsE": None,                               # trm_mixed_int16_kernel(MixOutArgs)
    "_ZN3trm27trm_mixed_file_image_kernelENS_10MixOutArgsE": None,                          # trm_mixed_file_image_kernel(MixOutArgs)
    "_ZN3trm16trm_noise_kernelEPfjjPd": None,                                               # trm_noise_kernel(float*, unsigned, unsigned, double*)
    # grouped streams: step tables, gain, int16 PCM
    "_ZN3trm19trm_grp_prep_kernelENS_11GrpPrepArgsE": None,                                 # trm_grp_prep_kernel(GrpPrepArgs)
    "_ZN3trm26trm_grp_prep_counts_kernelENS_17GrpPrepCountsArgsE": None,                    # trm_grp_prep_counts_kernel(GrpPrepCountsArgs)
    "_ZN3trm19trm_grp_gain_kernelENS_11GrpGainArgsE": None,                                 # trm_grp_gain_kernel(GrpGainArgs)
    "_ZN3trm20trm_grp_int16_kernelENS_12GrpInt16ArgsE": None,                               # trm_grp_int16_kernel(GrpInt16Args)
    "_ZN3trm25trm_grp_clip_clear_kernelEPjj": None,                                         # trm_grp_clip_clear_kernel(unsigned*, unsigned)
}


def named(stem):
    """the manifest's names that hold `stem` (the counts some tests keep: 8 of trm_tube_kernel, 6 of trm_mix_kernel)"""
    return [k for k in KERNELS if stem in k]


def check(kernels, *names):
    """each of `names` is a line of the manifest, and in `kernels` (kernel_notes.read_kernels) as that line says"""
    import kernel_notes
    for name in names:
        assert name in KERNELS, name
        kernel_notes.assert_within_budget(kernels, name, KERNELS[name])

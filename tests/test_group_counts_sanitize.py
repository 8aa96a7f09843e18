"""The host code of frame counts per group (trm_mixed_stream_step_counts and its int16 form) under AddressSanitizer and UBSan, on
the CPU: the library's host translation units and the CPU stand-ins of the HIP runtime are compiled, their host code instrumented
by both sanitizers and no device code with either, into a stand-alone program with its own main
(tests/_emul/group_counts_sanitize.cc), which drives create, the schedule of tests/group_counts_common.py through both host entries
under both conversion paths, a bind between steps, every refusal and destroy in both kernel forms, with frames that end at the
last counted row.  The program is run as it is: nothing is loaded into this interpreter."""
import os
import subprocess

import host_mock as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


def test_steps_with_counts_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "group_counts_sanitize")
    mocks = ("group_counts_sanitize.cc", "hip_host_mock.cc", "hip_host_mock_out.cc", "hip_host_mock_events.cc", "hip_host_mock_down.cc",
             "hip_host_mock_counts.cc")
    srcs = [os.path.join(ROOT, "tests", "_emul", f) for f in mocks]
    srcs += [os.path.join(CSRC, u + ".cc") for u in M.host_units()]
    oracle = os.path.join(ROOT, "oracle")        # (the track launcher's stand-in generates with the oracle's generator)
    if not os.path.exists(os.path.join(oracle, "libtrm_oracle.so")):
        subprocess.check_call(["make", "-s", "-C", oracle, "libtrm_oracle.so"])
    # (the sanitizers are the host compilation's alone: -Xarch_host in front of each of their options)
    subprocess.check_call(["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-L" + oracle, "-l:libtrm_oracle.so", "-Wl,-rpath," + oracle, "-lpthread", "-lm"])
    env = {k: v for k, v in os.environ.items() if k != "TRM_QUAD_CUS"}      # (the program chooses its kernel forms itself)
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "group_counts_sanitize: ok (instrumented)" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

"""The one-shot host entries (trm_batch_synthesize_host[_int16], trm_multi_synthesize_host, trm_mixed_synthesize_host[_int16],
trm_mixed_events_to_files_host) and the staging helpers they share under AddressSanitizer and UBSan, on the CPU: the library's host
translation units and the CPU stand-in of the HIP runtime are compiled, their host code instrumented by both sanitizers and no
device code with either, into a stand-alone program with its own main (tests/_emul/host_entries_sanitize.cc), which sweeps the
cases of tests/test_host_entries_ops.py in small, permuted and gapped ones among them.  The program is run as it is: nothing is
loaded into this interpreter."""
import os
import subprocess

import host_mock as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


def test_host_entries_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "host_entries_sanitize")
    srcs = [os.path.join(ROOT, "tests", "_emul", f) for f in ("host_entries_sanitize.cc", "hip_host_mock.cc")]
    srcs += [os.path.join(CSRC, u + ".cc") for u in M.host_units()]
    # (the sanitizers are the host compilation's alone: -Xarch_host in front of each of their options)
    subprocess.check_call(["hipcc", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-lpthread", "-lm"])
    env = {k: v for k, v in os.environ.items() if k not in ("TRM_QUAD_CUS", "TRM_TUBE_KERNEL", "TRM_TIME_SPLIT")}
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0 and "host_entries_sanitize: ok (instrumented)" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

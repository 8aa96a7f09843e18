"""The host build of the stage probes (tests/_probe/stage_probe_host.cc over the kernel headers' host stand-ins) under
AddressSanitizer and UBSan, on the CPU: a stand-alone program with its own main (tests/_probe/stage_probe_sanitize.cc) runs one
sweep of every probe with exactly sized buffers.  The program is run as it is: nothing is loaded into this interpreter."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


def test_probe_bodies_are_clean_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "stage_probe_sanitize")
    srcs = [os.path.join(ROOT, "tests", "_probe", f) for f in ("stage_probe_sanitize.cc", "stage_probe_host.cc")] + [os.path.join(CSRC, "trm_setup.cc")]
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe] + srcs + ["-lm"])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "stage_probe_sanitize: ok (instrumented)" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]

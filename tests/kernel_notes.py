"""The one reader of the kernels inside the built libtrm_hip.so: every gfx950 code object's notes (the AMDGPU metadata), one entry
per kernel built.  tests/kernel_manifest.py names the kernels the library is to hold; the checks on them are here."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gnuspeech_amd", "libtrm_hip.so")
OBJDUMP, READELF = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
VGPR_BUDGET = 128              # four waves per SIMD: what puts two workgroups on a CU

KEYS = {"scratch": r"\.private_segment_fixed_size", "sgpr_spills": r"\.sgpr_spill_count", "vgpr_spills": r"\.vgpr_spill_count",
        "vgprs": r"\.vgpr_count", "static_lds": r"\.group_segment_fixed_size"}

_read = {}


def tools_installed():
    return os.path.exists(OBJDUMP) and os.path.exists(READELF)


def read_kernels(lib_path=LIB):
    """{mangled name: [entry, ...]} over every gfx950 code object of the library, an entry per time the name is built, each a dict of
    KEYS' numbers.  Read once per process and state of the file; skips the calling test where the LLVM tools are missing."""
    if not tools_installed():
        pytest.skip("ROCm LLVM tools not installed")
    key = (os.path.abspath(lib_path), os.stat(lib_path).st_mtime_ns)
    if key not in _read:
        kernels = {}
        with tempfile.TemporaryDirectory() as tmp:
            lib = shutil.copy(lib_path, os.path.join(tmp, "lib.so"))
            subprocess.run([OBJDUMP, "--offloading", lib], check=True, capture_output=True, cwd=tmp)
            cos = [f for f in os.listdir(tmp) if "gfx950" in f]
            assert cos, "no gfx950 code object in %s" % os.path.basename(lib_path)
            for f in cos:
                notes = subprocess.run([READELF, "--notes", os.path.join(tmp, f)], check=True, capture_output=True, text=True).stdout
                for blk in notes.split("- .agpr_count:")[1:]:              # one metadata entry per kernel (its first key)
                    name = re.search(r"\.name:\s+(_Z\S+)", blk)
                    if name:
                        kernels.setdefault(name.group(1), []).append(
                            {k: int(re.search(pat + r":\s+(\d+)", blk).group(1)) for k, pat in KEYS.items()})
        _read[key] = kernels
    return _read[key]


def assert_within_budget(kernels, name, static_lds=None):
    """`name` is built exactly once, with no private segment, no spilled registers, at most VGPR_BUDGET VGPRs and, where one is
    given, that much static LDS"""
    assert name in kernels, (name, sorted(kernels))
    assert len(kernels[name]) == 1, (name, "built %d times" % len(kernels[name]))
    e = kernels[name][0]
    print("%s: scratch %d, SGPR spills %d, VGPR spills %d, VGPRs %d, static LDS %d"
          % (name, e["scratch"], e["sgpr_spills"], e["vgpr_spills"], e["vgprs"], e["static_lds"]))
    assert e["scratch"] == 0 and e["sgpr_spills"] == 0 and e["vgpr_spills"] == 0, (name, e)
    assert e["vgprs"] <= VGPR_BUDGET, (name, e["vgprs"])
    if static_lds is not None:
        assert e["static_lds"] == static_lds, (name, e["static_lds"])

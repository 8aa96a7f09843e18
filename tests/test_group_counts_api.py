"""CPU-side checks of frame counts per group (include/trm_c_api.h: trm_mixed_stream_step_counts and its device and int16 forms): the
four entries are exported and declared with a count array and a frame pitch, the Python methods take `counts`, the room of the
step's tables covers the counts stretch, and the kernel that lays the rows out per count is in the library."""
import inspect
import os
import re
import subprocess

import kernel_manifest
import kernel_notes
import support

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")
NEW = ["trm_mixed_stream_step_counts", "trm_mixed_stream_step_counts_device", "trm_mixed_stream_step_counts_int16",
       "trm_mixed_stream_step_counts_device_int16"]

g = support.product(gpu=False)


def test_the_four_entries_are_exported_and_declared(g):
    header = open(os.path.join(ROOT, "include", "trm_c_api.h")).read()
    for name in NEW:
        assert name in g._capi.EXPORTS, name
        m = re.search(r"int\s+%s\(([^;]*)\);" % name, header)
        assert m, name
        args = " ".join(m.group(1).split())
        # today's entry with a count per group and a row pitch in place of nframes
        assert "const uint32_t *count" in args and "size_t frame_pitch" in args and "nframes" not in args, (name, args)
        assert ("hip_stream" in args) == ("device" in name) and ("level" in args) == ("int16" in name), (name, args)
        fn = getattr(g.lib(), name)
        old = getattr(g.lib(), name.replace("_counts", ""))
        assert len(fn.argtypes) == len(old.argtypes) + 1, name
    assert "Frame counts per group" in header


def test_a_null_stream_is_refused(g):
    L, E = g.lib(), g._capi.TRM_EINVAL
    assert L.trm_mixed_stream_step_counts(None, None, None, None, 0, None, 0, None, None) == E
    assert L.trm_mixed_stream_step_counts_device(None, None, None, None, 0, None, 0, None, None, None) == E
    assert L.trm_mixed_stream_step_counts_int16(None, None, None, None, 0, None, 0, None, 0, None, None, None) in (E, g._capi.TRM_EHIP)
    assert L.trm_mixed_stream_step_counts_device_int16(None, None, None, None, 0, None, 0, None, 0, None, None, None, None) in (E, g._capi.TRM_EHIP)


def test_the_python_methods_take_counts(g):
    """step and step_device by the keyword counts=None; the int16 steps, whose parameter lists tests/test_group_int16_api.py pins,
    by methods of their own with `counts` behind `actions`"""
    for name in ("step", "step_device"):
        p = inspect.signature(getattr(g.TRMGroupedStream, name)).parameters
        assert "counts" in p and p["counts"].default is None, name
    for name in ("step_counts_int16", "step_counts_device_int16"):
        assert list(inspect.signature(getattr(g.TRMGroupedStream, name)).parameters)[:3] == ["self", "actions", "counts"], name
        old = list(inspect.signature(getattr(g.TRMGroupedStream, name.replace("_counts", ""))).parameters)
        assert "counts" not in old and sorted(inspect.signature(getattr(g.TRMGroupedStream, name)).parameters) == sorted(old + ["counts"]), name
    assert callable(g.TRMGroupedStream._group_counts)


def test_the_room_of_the_steps_tables_covers_the_counts_stretch(tmp_path):
    """step_words_room with the counts stretch is the room without it plus a word per group, whatever other stretches the stream
    has made room for, and step_layout at its maxima ends exactly there, the counts stretch last"""
    exe = str(tmp_path / "group_counts_layout")
    subprocess.check_call(["hipcc", "-O1", "-std=c++17", "-fno-exceptions", os.path.join(ROOT, "tests", "_emul", "group_counts_layout.cc"), "-o", exe])
    rows = [[int(x) for x in ln.split()] for ln in subprocess.check_output([exe], text=True).splitlines()]
    assert len(rows) == 4 and len({r[0] for r in rows}) == 4
    for without, with_, at, words in rows:
        assert with_ == without + 3 and at == without and words == with_
    # a stream that never takes a step with counts keeps its tables: the engine asks for the stretch only once it has
    src = open(os.path.join(CSRC, "trm_stream_step.cc")).read()
    assert "step_words_room(s, s->downRoom, s->perSet, s->countsRoom)" in src and "s->countsRoom = true" in src
    assert "step_words_room(s, false, false, false)" in open(os.path.join(CSRC, "trm_stream.cc")).read()


def test_the_kernel_is_in_the_library():
    """trm_grp_prep_counts_kernel once in the gfx950 code objects of libtrm_hip.so, beside trm_grp_prep_kernel, without scratch or
    spills (tests/test_capi_exports.py holds that for every kernel; here the new one is looked at by name)"""
    assert kernel_notes.tools_installed(), "ROCm LLVM tools are needed to look into the library's code objects"
    assert "trm_grp_prep.hip" in open(os.path.join(CSRC, "Makefile")).read()
    found = kernel_manifest.named("trm_grp_prep")
    assert sorted("counts" in n for n in found) == [False, True], found
    kernel_manifest.check(kernel_notes.read_kernels(), *found)

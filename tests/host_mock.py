"""What the tests on the CPU stand-in of the HIP runtime (tests/_emul/hip_host_mock.cc) share: its checking heap seen from Python.
The stand-in records every hipMalloc / hipHostMalloc block with guard zones around it, refuses copies, memsets and kernel spans
that leave a block, and counts each refusal as a violation; these helpers read that count, walk the guards, and give a test
"device" memory of its own (a block of the stand-in's heap viewed as a numpy array) for the entries that take device pointers."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gnuspeech_amd", "csrc")


def carried_parts(csrc=CSRC):
    """the .cc files of `csrc` that another .cc of it carries with an #include (the parts of trm_stream.cc): no units of their own"""
    files = [f for f in os.listdir(csrc) if f.endswith(".cc")]
    return sorted({m for f in files for m in re.findall(r'^#include "(\w+\.cc)"', open(os.path.join(csrc, f)).read(), re.M)})


def host_units(csrc=CSRC):
    """the library's host translation units: the .cc files of `csrc` but for carried_parts, by name without the suffix.  Read from
    the directory, so that another commit's tree (a golden's recording) gives that commit's units."""
    return sorted(f[:-3] for f in os.listdir(csrc) if f.endswith(".cc") and f not in carried_parts(csrc))


def unit_dependencies(csrc=CSRC):
    """what every unit's object may depend on besides its own .cc: the headers, the carried parts and the public header"""
    return [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h") or f in carried_parts(csrc)] + [os.path.join(ROOT, "include", "trm_c_api.h")]


H2D, D2H, D2D = 1, 2, 3                      # hipMemcpyKind
EINVALID = 1                                 # hipErrorInvalidValue


def bind(L):
    """argument and result types of the stand-in's own entries (idempotent)"""
    L.mock_violations.argtypes, L.mock_violations.restype = [C.c_char_p, C.c_size_t], C.c_int
    L.mock_check_heap.argtypes, L.mock_check_heap.restype = [], C.c_int
    L.mock_fail_malloc.argtypes, L.mock_fail_malloc.restype = [C.c_int, C.c_int], None
    L.mock_malloc_count.argtypes, L.mock_malloc_count.restype = [], C.c_long
    L.hipMalloc.argtypes, L.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    L.hipHostMalloc.argtypes, L.hipHostMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t, C.c_uint], C.c_int
    L.hipFree.argtypes, L.hipFree.restype = [C.c_void_p], C.c_int
    L.hipHostFree.argtypes, L.hipHostFree.restype = [C.c_void_p], C.c_int
    L.hipMemcpy.argtypes, L.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    L.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
    L.hipMemcpy2DAsync.restype = C.c_int
    L.hipMemset.argtypes, L.hipMemset.restype = [C.c_void_p, C.c_int, C.c_size_t], C.c_int
    L.hipGetErrorString.argtypes, L.hipGetErrorString.restype = [C.c_int], C.c_char_p
    return L


def violations(L):
    """(count since the last call, the first one's text)"""
    buf = C.create_string_buffer(512)
    n = bind(L).mock_violations(buf, len(buf))
    return n, buf.value.decode()


def assert_clean(L):
    """no violations since the last look, and every guard zone of the heap intact"""
    damaged = bind(L).mock_check_heap()
    n, first = violations(L)
    assert damaged == 0 and n == 0, "%d violations of the stand-in's heap, %d blocks with damaged guards; first: %s" % (n, damaged, first)


class DeviceArray:
    """a hipMalloc block of the stand-in as a numpy array `a` of exactly the block's size; free() verifies its guards"""

    def __init__(self, L, shape, dtype, fill=None):
        self._L = bind(L)
        shape = (shape,) if np.isscalar(shape) else tuple(shape)
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        assert self._L.hipMalloc(C.byref(p), n) == 0
        self.ptr = p.value
        self.a = np.frombuffer((C.c_char * n).from_address(self.ptr), dtype=dtype).reshape(shape)
        if fill is not None:
            self.a[...] = fill

    def free(self):
        if self.ptr:
            self.a = None
            assert self._L.hipFree(self.ptr) == 0
            self.ptr = None

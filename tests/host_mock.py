"""What the tests on the CPU stand-in of the HIP runtime (tests/_emul/hip_host_mock.cc) share: its checking heap seen from Python.
The stand-in records every hipMalloc / hipHostMalloc block with guard zones around it, refuses copies, memsets and kernel spans
that leave a block, and counts each refusal as a violation; these helpers read that count, walk the guards, and give a test
"device" memory of its own (a block of the stand-in's heap viewed as a numpy array) for the entries that take device pointers.
Also how such a library comes about and is used: build() links the host units over a module's stand-ins (each module keeps its
own MOCKS and WRAPPED lists), product_on() / load() bind the package to it, trace_take() reads a recorder, heap_clean() makes
the autouse fixture that checks the heap after every test."""
import contextlib
import ctypes as C
import gc
import os
import re
import subprocess

import numpy as np
import pytest

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


def build(out, mocks, wrapped=(), csrc=CSRC, oracle=False, reuse_objects=False):
    """the host units of `csrc` as the shared library `out`, over the stand-ins `mocks` (files of tests/_emul), the symbols `wrapped`
    behind the recorder among them (-Wl,--wrap), linked with the oracle's library where a stand-in calls it.  reuse_objects: the
    product build's host objects where they are fresh, so that only the stand-ins are compiled."""
    srcs = [os.path.join(csrc, u + ".cc") for u in host_units(csrc)]
    mocks = [os.path.join(ROOT, "tests", "_emul", m) for m in mocks]
    link = ["-lpthread", "-lm"]
    if oracle:
        odir = os.path.join(ROOT, "oracle")
        if not os.path.exists(os.path.join(odir, "libtrm_oracle.so")):
            subprocess.check_call(["make", "-s", "-C", odir, "libtrm_oracle.so"])
        link = ["-L" + odir, "-l:libtrm_oracle.so", "-Wl,-rpath," + odir] + link
    flags = ["-O1", "-std=c++17", "-fPIC"]
    # (-Bsymbolic: the library's calls into the runtime bind to the stand-in, whatever else the process has loaded)
    shared = ["-shared", "-Wl,-Bsymbolic", "-o", out] + ["-Wl,--wrap=" + w for w in wrapped]
    objs = [os.path.join(csrc, "build", u + ".o") for u in host_units(csrc)]
    if reuse_objects and all(os.path.exists(o) and all(os.path.getmtime(o) >= os.path.getmtime(d) for d in [s] + unit_dependencies(csrc))
                             for o, s in zip(objs, srcs)):
        mos = ["%s.%d.o" % (out[:-3], i) for i in range(len(mocks))]
        for m, mo in zip(mocks, mos):
            subprocess.check_call(["hipcc"] + flags + ["-c", m, "-o", mo])
        subprocess.check_call(["g++"] + shared + mos + objs + link)
    else:
        subprocess.check_call(["hipcc"] + flags + shared + mocks + srcs + link)


@contextlib.contextmanager
def product_on(lib_path):
    """gnuspeech_amd bound to the stand-in library at `lib_path` (one "device"), and back to what it was bound to afterwards"""
    import gnuspeech_amd
    from gnuspeech_amd import _capi
    saved = (_capi._lib, _capi.LIB_PATH)
    _capi._lib, _capi.LIB_PATH = None, lib_path
    try:
        assert _capi.lib().trm_device_count() == 1
        yield gnuspeech_amd
    finally:
        gc.collect()             # (streams of the stand-in are destroyed by the stand-in)
        _capi._lib, _capi.LIB_PATH = saved


def load(lib_path):
    """gnuspeech_amd's ctypes view of the stand-in library at `lib_path` (argument types included, the stand-in's own entries too);
    the package itself stays bound to what it was"""
    with product_on(lib_path) as pkg:
        return bind(pkg.lib())


def c_params(pd):
    """the C structure of the input parameters in the dict `pd`"""
    from gnuspeech_amd import TRMInputParameters
    return TRMInputParameters.from_dict(pd).c


def set_begin_of(sets, V):
    """set_begin of V voices dealt evenly over `sets`; of five sets the third stays empty"""
    live = [s for s in range(len(sets)) if not (len(sets) == 5 and s == 2)]
    counts = [0] * len(sets)
    for i, s in enumerate(live):
        counts[s] = V // len(live) + (1 if i < V % len(live) else 0)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)


def trace_take(L, lines=True):
    """what the recorder (a hip_op_trace*.cc) wrote down since the last call, as lines or as one text"""
    L.trace_take.argtypes, L.trace_take.restype = [C.c_char_p, C.c_size_t], C.c_size_t
    n = L.trace_take(None, 0)
    buf = C.create_string_buffer(n + 1)
    L.trace_take(buf, n + 1)
    text = buf.value.decode()
    return text.splitlines() if lines else text


def heap_clean(before_check=None):
    """an autouse fixture over the module's `g`: every test is a bounds test too -- the stand-in's checking heap saw no copy, memset
    or kernel span leave its block, and no guard zone was written.  before_check(L) puts back what a test may have left set."""
    @pytest.fixture(autouse=True)
    def fixture(g):
        violations(g.lib())
        yield
        if before_check is not None:
            before_check(g.lib())
        gc.collect()
        assert_clean(g.lib())
    return fixture


def allow_malloc(L):
    """heap_clean's before_check of the modules that make hipMalloc fail: it succeeds again"""
    bind(L).mock_fail_malloc(0, 0)


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

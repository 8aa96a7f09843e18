"""What the CPU tests of the time split's form setting share (tests/test_split_oct_api.py, tests/test_split_oct_plan_host.py): the
library's host translation units on the CPU stand-in of the HIP runtime with the one-shot launches' recorder in front, built once per
process by tests/test_split_plan_host.py's own recipe (both files of tests/_emul as they are)."""
import functools
import os
import tempfile

import host_mock as M
import test_split_plan_host as P


@functools.lru_cache(maxsize=None)
def mock_library():
    out = os.path.join(tempfile.mkdtemp(prefix="hostmock_split_oct_"), "libtrm_hostmock_split_oct.so")
    M.build(out, P.MOCKS, P.WRAPPED)
    L = M.load(out)
    P.warm_noise(L)
    return L

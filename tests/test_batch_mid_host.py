"""Mid-size members of a batch, host side (no GPU): the two new entry points are declared in the header and exported, the ABI
version is unchanged, and the ctypes binding declares their signatures."""
import ctypes as C
import os
import re

from cyclistsocialforce_amd import _ffi
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_batch_mid_ticks", "csf_batch_launches")


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
        assert re.search(r"int\s+%s\(const csf_engine \*e, int64_t \*\w+\);" % s, header), s
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9
    assert re.search(r"#define\s+CSF_ABI_VERSION\s+9\b", header)


def test_ctypes_signatures():
    lib = _ffi.load()
    for s in NEW:
        assert getattr(lib, s).argtypes == [C.c_void_p, C.POINTER(C.c_int64)], s
        assert getattr(lib, s).restype in (C.c_int, C.c_int32), s


def test_null_arguments_are_refused_without_a_device():
    lib = _ffi.load()
    n = C.c_int64(5)
    for s in NEW:
        assert getattr(lib, s)(None, C.byref(n)) == -1 and n.value == 5, s
    assert callable(Engine.batch_mid_ticks) and callable(Engine.batch_launches)

"""Force-field maps (include/csf.h: csf_field_map), the parts that need no GPU: the header, the library's exports, the
Python bindings and the argument checks that run before any device call."""
import os
import re
import sys

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "csf.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def test_header_declares_the_two_functions_and_the_three_flags():
    h = header_text()
    assert re.search(r"int\s+csf_field_map\s*\(\s*csf_engine\s*\*\s*e\s*,\s*int64_t\s+m\s*,\s*const\s+double\s*\*\s*x\s*,\s*const\s+double\s*\*\s*y\s*,"
                     r"\s*const\s+double\s*\*\s*psi\s*,\s*uint32_t\s+what\s*,\s*int32_t\s+skip\s*,\s*double\s*\*\s*Fx\s*,\s*double\s*\*\s*Fy\s*\)\s*;", h)
    assert re.search(r"int\s+csf_field_map_launches\s*\(\s*const\s+csf_engine\s*\*\s*e\s*,\s*int64_t\s*\*\s*n_launches\s*\)\s*;", h)
    for name, value in (("CSF_FIELD_CROWD", "1u"), ("CSF_FIELD_ROAD", "2u"), ("CSF_FIELD_FOV", "4u")):
        assert re.search(rf"#define\s+{name}\s+{value}\b", h), name
    assert (_ffi.FIELD_CROWD, _ffi.FIELD_ROAD, _ffi.FIELD_FOV) == (1, 2, 4)


def test_abi_version_stays_9():
    assert re.search(r"#define\s+CSF_ABI_VERSION\s+9\b", header_text())
    assert _ffi.ABI_VERSION == 9


def test_symbols_list_names_them():
    assert "csf_field_map" in _ffi.SYMBOLS and "csf_field_map_launches" in _ffi.SYMBOLS


def test_library_exports_them_and_is_abi_9():
    lib = _ffi.load()
    assert hasattr(lib, "csf_field_map") and hasattr(lib, "csf_field_map_launches")
    assert lib.csf_abi_version() == 9


@pytest.mark.parametrize("x,y,psi,kw", [
    (np.zeros((3, 4)), np.zeros((4, 3)), 0.0, {}),                       # x against y
    (np.zeros(5), np.zeros(6), None, dict(crowd=False)),
    (np.zeros((3, 4)), np.zeros((3, 4)), np.zeros(12), {}),              # psi against x
    (np.zeros(5), np.zeros(5), np.zeros(4), {}),
    (np.zeros(5), np.zeros(5), None, {}),                                # the crowd term without headings
    (np.zeros(5), np.zeros(5), 0.0, dict(crowd=False, road=False)),      # no term
    (np.zeros(5), np.zeros(5), 0.0, dict(crowd=False, fov=True)),        # the mask without the crowd term
])
def test_shape_mismatches_raise_before_any_device_call(x, y, psi, kw):
    e = Engine.__new__(Engine)          # no handle, no library: whatever touched the device would raise AttributeError
    with pytest.raises(ValueError):
        Engine.field_map(e, x, y, psi, **kw)


def test_road_elements_have_the_reference_methods():
    from cyclistsocialforce_amd import intersection
    for cls in (intersection.RoadEdge, intersection.RoadSegment, intersection.RoadSegmentCollection):
        assert callable(getattr(cls, "calcRepulsiveForce"))
    assert callable(intersection.SocialForceIntersection.force_field)
    sys.path.insert(0, os.path.join(ROOT, "compat"))          # the drop-in package exposes the same classes
    before = set(sys.modules)
    try:
        import cyclistsocialforce.intersection as compat
        for cls in (intersection.RoadEdge, intersection.RoadSegment, intersection.RoadSegmentCollection, intersection.SocialForceIntersection):
            assert getattr(compat, cls.__name__) is cls
    finally:
        sys.path.remove(os.path.join(ROOT, "compat"))
        for name in set(sys.modules) - before:                 # (leave no `cyclistsocialforce` behind for the tests that follow)
            if name.split(".")[0] == "cyclistsocialforce":
                del sys.modules[name]

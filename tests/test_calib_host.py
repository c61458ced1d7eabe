"""Calibration, host side (no GPU): the entry points are declared, exported and bound; the error functions are the reference's
formulas; CalibrationData iterates and partitions; the ask / tell downhill simplex is scipy.optimize.fmin to the last bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy.optimize import fmin

from cyclistsocialforce_amd import _ffi, calibration as cal
from cyclistsocialforce_amd.engine import Engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("csf_calib_load", "csf_calib_eval", "csf_calib_launches", "csf_calib_clear")


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "csf.h")).read()
    declared = set(re.findall(r"\b(csf_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load()
    for s in NEW:
        assert s in declared and s in _ffi.SYMBOLS and hasattr(lib, s), s
    assert lib.csf_abi_version() == 9 and _ffi.ABI_VERSION == 9
    assert re.search(r"#define\s+CSF_ABI_VERSION\s+9\b", header)


def test_ctypes_signatures():
    lib = _ffi.load()
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    assert lib.csf_calib_load.argtypes == [vp, i32, i64, vp, vp, vp, vp, vp, i32, vp, i32]
    assert lib.csf_calib_eval.argtypes == [vp, i32, C.POINTER(_ffi.Params), C.c_size_t, i32, i32, vp, i32, vp]
    assert lib.csf_calib_launches.argtypes == [vp, C.POINTER(i64)]
    assert lib.csf_calib_clear.argtypes == [vp]
    for s in NEW:
        assert getattr(lib, s).restype in (C.c_int, C.c_int32), s


def test_null_engine_is_refused_without_a_device():
    lib = _ffi.load()
    n = C.c_int64(5)
    a = np.zeros(8)
    f = np.zeros(1, dtype=np.int32)
    p = a.ctypes.data_as(C.c_void_p)
    assert lib.csf_calib_load(None, 1, 1, p, p, p, None, p, 1, f.ctypes.data_as(C.c_void_p), 1) == -1
    pod = _ffi.Params()
    assert lib.csf_calib_eval(None, 1, C.byref(pod), C.sizeof(pod), 9, 1, p, 1, None) == -1
    assert lib.csf_calib_launches(None, C.byref(n)) == -1 and n.value == 5
    assert lib.csf_calib_clear(None) == -1
    for m in ("calib_load", "calib_eval", "calib_clear", "calib_launches"):
        assert callable(getattr(Engine, m)), m


def test_compat_module_re_exports():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "compat"))
    try:
        from cyclistsocialforce import calibration as c2
    finally:
        sys.path.pop(0)
    for name in ("calc_sse_timesteps", "calc_maesse_samples", "CalibrationData", "DownhillSimplexCalibration"):
        assert getattr(c2, name) is getattr(cal, name), name


def test_error_functions_are_the_references_formulas():
    rng = np.random.default_rng(3)
    outs = [rng.normal(size=(n, 3)) for n in (7, 19, 1)]
    objs = [o + rng.normal(size=o.shape) for o in outs]
    sse = sum(float(((o - b) ** 2).sum()) for o, b in zip(outs, objs))
    mae = sum(float(np.abs(o - b).mean()) ** 2 for o, b in zip(outs, objs))
    assert cal.calc_sse_timesteps(outs, objs) == pytest.approx(sse, rel=1e-15)
    assert cal.calc_maesse_samples(outs, objs) == pytest.approx(mae, rel=1e-15)


def _tracks(rng, n=10):
    keys = ["Fx", "Fy", "x", "y", "psi", "v"]
    return [rng.normal(size=(int(rng.integers(5, 30)), 6)) for _ in range(n)], keys


def test_calibration_data_iteration_and_partition():
    rng = np.random.default_rng(5)
    tracks, keys = _tracks(rng)
    data = cal.CalibrationData(tracks, [0, 0, 0, 0, 1, 0], [1, 1, 0, 0, 0, 0], feature_keys=keys)
    seen = 0
    for trk, (s0, inp, obj) in zip(tracks, data):
        assert s0.shape == (6,) and np.array_equal(s0[:4], trk[0, 2:6]) and s0[4] == 0 and s0[5] == 0
        assert inp.shape == (trk.shape[0] - 1, 2) and np.array_equal(inp, trk[1:, :2])
        assert obj.shape == (trk.shape[0] - 1, 1) and np.array_equal(obj[:, 0], trk[1:, 4])
        seen += 1
    assert seen == len(tracks) and len(list(data)) == len(tracks)          # (a second iteration starts over)
    a, b = data.partition(2, [0.7, 0.3], random_seed=1)
    assert (len(a), len(b)) == (7, 3)
    a2, b2 = data.partition(2, [0.7, 0.3], random_seed=1)
    assert [id(t) for t in a.tracks] == [id(t) for t in a2.tracks]            # seeded: the same split
    assert sorted(id(t) for t in a.tracks + b.tracks) == sorted(id(t) for t in data.tracks)
    assert np.array_equal(a.objective_features, data.objective_features)
    with pytest.raises(ValueError):
        cal.CalibrationData(tracks, [1, 0], [1, 1, 0, 0, 0, 0], feature_keys=keys)


def _quadratic(x):
    return float((x[0] - 1.5) ** 2 + 3.0 * (x[1] + 0.5) ** 2 + 0.5 * x[0] * x[1])


def _rosenbrock(x):
    return float(100.0 * (x[1] - x[0] ** 2) ** 2 + (1.0 - x[0]) ** 2 + (0.0 if len(x) < 3 else 100.0 * (x[2] - x[1] ** 2) ** 2 + (1.0 - x[1]) ** 2))


CASES = [(_quadratic, [0.3, 0.2], 100), (_quadratic, [0.0, -2.0], 500), (_rosenbrock, [-1.2, 1.0], 100), (_rosenbrock, [-1.2, 1.0], 1000),
         (_rosenbrock, [0.5, 0.0, 2.0], 800), (_rosenbrock, [2.0, 2.0], 7)]


@pytest.mark.parametrize("func,x0,maxiter", CASES)
def test_ask_tell_simplex_is_scipy_fmin_exactly(func, x0, maxiter):
    xopt, fopt, it, _, _ = fmin(func, x0, full_output=True, maxiter=maxiter, disp=False)
    (x, f, n), = cal.minimize_many(lambda pts: [func(p) for p in pts], [x0], maxiter=maxiter)
    assert np.array_equal(x, xopt) and f == fopt and n == it


def test_maxiter_must_be_given():
    with pytest.raises(ValueError):
        cal.NelderMead([1.0, 2.0])


def test_params_args_dict_and_auxiliary_functions():
    c = cal.DownhillSimplexCalibration.__new__(cal.DownhillSimplexCalibration)
    c.params_keys, c.params_auxfuncs, c.params_auxfuncsargs = ["a", "b"], None, None
    assert c._update_params_args_dict([1.0, 2.0]) == {"a": 1.0, "b": 2.0}
    c.params_auxfuncs, c.params_auxfuncsargs = [lambda v, s=1: s * v[0], lambda v: v[0] + v[1]], [{"s": 3}, {}]
    assert c._update_params_args_dict([1.0, 2.0]) == {"a": 3.0, "b": 3.0}
    with pytest.raises(ValueError):
        cal.DownhillSimplexCalibration(None, ["a", "b"], None, None, [1, 0, 0, 0, 0, 0], params_auxfuncs=[abs])


def test_run_many_lockstep_equals_separate_runs():
    rng = np.random.default_rng(11)
    starts = [rng.uniform(-2, 2, 2) for _ in range(5)]
    calls = []

    def many(pts):
        calls.append(len(pts))
        return [_rosenbrock(p) for p in pts]

    together = cal.minimize_many(many, starts, maxiter=150)
    for g, (x, f, n) in zip(starts, together):
        (x1, f1, n1), = cal.minimize_many(lambda pts: [_rosenbrock(p) for p in pts], [g], maxiter=150)
        xs, fs, ns, _, _ = fmin(_rosenbrock, g, full_output=True, maxiter=150, disp=False)
        assert np.array_equal(x, x1) and f == f1 and n == n1
        assert np.array_equal(x, xs) and f == fs and n == ns
    assert calls[0] == 5 * 3 and max(calls[1:]) <= 5 * 4       # every round of all live runs is ONE call

"""cyclistsocialforce_amd/calibration.py against the real engine, before and after the module was split into layers (DESIGN.md 4.10,
the Python layering): what tests/calibration_calls_common.py's recording engine cannot show - the engine's own state width, the NaN
rows of shared lanes, the widest state under mixed classes.  Eight small data sets (10 - 20 ticks, max_sets = 2, three vectors, so two
launches per evaluation): `evaluate` under both built-in error functions and a custom one, and `simulate`.  The fixture
tests/golden/calibration_py_gpu.npz was recorded on an MI355X with calibration.py as it was before the split
(tests/golden/make_golden_calibration_py_gpu.py); the device library is the same, so the assertion is array_equal, NaN in the same
places."""
import os

import numpy as np
import pytest

from calibration_calls_common import custom_error
from scene_calib_common import crowd

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT = [1, 1, 0, 1, 0, 0]
T_S = 0.01


def scene(seed, n, ticks, box=14.0, width=5, **kw):
    """n road users of crowd() and a recording that drifts along their heading, with noise: an objective no candidate meets"""
    from cyclistsocialforce_amd import calibration as cal
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    rng = np.random.default_rng(1000 + seed)
    s0 = np.zeros((n, width))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    t = (np.arange(ticks) + 1.0)[:, None]
    traj = np.stack([x + T_S * t * v * np.cos(psi), y + T_S * t * v * np.sin(psi), psi + 0.0 * t, v + 0.0 * t], axis=2)
    traj += 0.05 * rng.normal(size=traj.shape)
    return cal.SceneData(s0, rng.uniform(4.0, 6.0, size=n), off, dq, traj, **kw)


def _road(box=14.0):
    verts = np.r_[np.c_[np.linspace(-5.0, box + 5.0, 40), np.full(40, -2.0)], np.c_[np.linspace(-5.0, box + 5.0, 25), np.full(25, box + 2.0)]]
    return [0, 40, 65], verts, [6.0, 5.0], [2.0, 2.5]


def _roster34(**kw):
    return scene(3, 34, 20, box=30.0, present=(np.arange(34) // 2, np.arange(34) // 2 + 3), **kw)


def _two(group):
    from cyclistsocialforce_amd import vehicle
    return dict(vtype=[vehicle.TwoDBicycle, vehicle.InvPendulumBicycle], keys=[("f_0", 0), ("f_0", 1), "sigma_0"], base=[7.0, 9.0, 0.5],
                data=[scene(8, 4, 14, box=8.0, width=8, group=group), scene(9, 3, 10, box=8.0, width=6, group=[1, 0, 1])])


GROUPED = dict(keys=[("f_0", 0), ("f_0", 1), "sigma_0"], base=[7.0, 9.0, 0.5], group_params=[dict(hfov=2.0), dict(hfov=3.0, e_0=0.9)])

CASES = {
    "plain": lambda: dict(data=[scene(1, 3, 16, length=13), scene(2, 5, 12)]),
    "replay_windows": lambda: dict(data=[scene(4, 6, 16, replayed=np.arange(6) == 4,
                                               present=([0, 3, 8, 0, 2, 5], [16, 12, 8, 9, 14, 16]))] + scene(5, 3, 12, box=8.0).ego_split()),
    "road_keys": lambda: dict(keys=["f_0", "road_F_0", "road_sigma"], base=[7.0, 0.15, 2.5], data=[scene(6, 4, 14, road=_road()), scene(7, 3, 10)]),
    "shared": lambda: dict(data=[_roster34(), scene(2, 5, 12)]),
    "wide": lambda: dict(data=[scene(10, 40, 12, box=34.0, wide=True), scene(2, 5, 12)]),
    "groups": lambda: dict(data=[scene(1, 3, 16, length=13, group=[0, 1, 1]), scene(2, 5, 12, group=[1, 0, 1, 0, 0])], **GROUPED),
    "lane_groups": lambda: dict(data=[_roster34(group=np.arange(34) % 2), scene(2, 5, 12, group=[1, 0, 1, 0, 0])], lane_groups=True, **GROUPED),
    "two_classes": lambda: _two([0, 1, 0, 1]),
}
FUNCS = ("calc_sse_timesteps", "calc_maesse_samples", "custom")


def run_case(name):
    """{label: array} of one case: the errors of three vectors under every error function, the scenes of simulate and the objectives"""
    from cyclistsocialforce_amd import calibration as cal, vehicle
    spec = dict(vtype=vehicle.TwoDBicycle, keys=["f_0", "sigma_0"], base=[7.0, 0.5])
    spec.update(CASES[name]())
    vtype, keys, base, data = (spec.pop(k) for k in ("vtype", "keys", "base", "data"))
    vectors = np.asarray(base)[None, :] * (1.0 + 0.1 * np.arange(3))[:, None]
    out = {}
    for label in FUNCS:
        func = custom_error if label == "custom" else getattr(cal, label)
        c = cal.InteractionCalibration(vtype, keys, data, data, FEAT, error_func=func, max_sets=2, **spec)
        out[label] = c.evaluate(vectors)
        if label == "custom":
            trajs, objs = c.simulate(vectors[1])
            for q, (t, o) in enumerate(zip(trajs, objs)):
                out[f"traj{q}"], out[f"obj{q}"] = t, o
        c.close()
    return out


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(HERE, "golden", "calibration_py_gpu.npz"))


@pytest.mark.parametrize("name", list(CASES))
def test_errors_and_trajectories_are_the_recorded_ones(recorded, name):
    got = run_case(name)
    want = {k[len(name) + 2:]: recorded[k] for k in recorded.files if k.startswith(name + "__")}
    assert sorted(got) == sorted(want) and len(got) > len(FUNCS)
    for label in got:
        assert got[label].shape == want[label].shape and np.array_equal(got[label], want[label], equal_nan=True), f"{name}: {label}"
    assert all(np.isfinite(got[label]).all() and np.all(got[label] > 0) for label in FUNCS)

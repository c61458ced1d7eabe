"""Closed-loop scene calibration on scenes with road edges: csf_scene_calib_road / csf_scene_calib_eval_road against
stand-alone engines that hold a scene and its road, the oracle, the refusals, and the optimiser on top of it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import scene_road_common as rc
from scene_calib_common import MODELS, VDES, oracle_case
from test_gpu_scene_calib import _check_sums, _sums_reference

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 1, 2], dtype=np.int32)
CONFIGS = [(m, 0) for m in MODELS] + [("twod", 1)]
ROFF = np.r_[0, np.cumsum(rc.N_RIDERS)]
_cache = {}


def _dataset(model, rule):
    """the data set of scene_road_common for one class and priority rule, loaded with its roads; computed once per configuration:
    (sets, per-scene (s0, off, dq), objective, sums and states of the evaluation with the roads' own parameters, the same without roads)"""
    key = (model, rule)
    if key not in _cache:
        from cyclistsocialforce_amd.engine import Engine
        sets = rc.rule_sets(model, rule)
        s0, off, rows, per = rc.scenes(model, rc.N_RIDERS, seed=MODELS.index(model), short=(rc.SHORT,))
        R, K = s0.shape[0], len(sets)
        obj = np.random.default_rng(3).normal(size=(rc.T, R, len(FEAT)))
        e = Engine(sets[0], K * R)
        e.scene_calib_load(rc.N_RIDERS, s0, VDES, off, rows, obj, FEAT, lengths=rc.LENGTHS, max_sets=K)
        bare = e.scene_calib_eval(sets, states=True)
        e.scene_calib_road(*rc.road_args(model))
        road = e.scene_calib_eval(sets, states=True)
        for a in bare + road:
            a.setflags(write=False)
        _cache[key] = dict(engine=e, sets=sets, per=per, obj=obj, R=R, K=K, bare=bare, road=road, load=(s0, off, rows))
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for ds in _cache.values():
        ds["engine"].close()
    _cache.clear()


def _against_twins(ds, model, sums, states, over=None):
    """every (set, scene) against a stand-alone engine that holds the set, the scene and its road (with the set's road parameters on
    every edge where `over` gives them): states within 2e-7, pointers and navigation state equal; returns the largest difference"""
    R, K = ds["R"], ds["K"]
    _, ptr_e, zn_e, _ = ds["engine"].state(with_nav=True)
    ptr_e, zn_e = np.asarray(ptr_e).reshape(-1)[: K * R].reshape(K, R), np.asarray(zn_e).reshape(-1, 3)[: K * R].reshape(K, R, 3)
    worst = np.zeros(len(rc.N_RIDERS))
    for k, pod in enumerate(ds["sets"]):
        for q, (sq, oq, dq) in enumerate(ds["per"]):
            ln = int(rc.LENGTHS[q])
            road = rc.road_of(model, q) if over is None else rc.road_of(model, q, *over[k])
            tw, ptr, zn = rc.twin_road(pod, sq, oq, dq, ln, road)
            got = states[:ln, k * R + ROFF[q]: k * R + ROFF[q + 1]]
            worst[q] = max(worst[q], float(np.abs(got - tw).max()))
            np.testing.assert_allclose(got, tw, rtol=2e-7, atol=2e-7, err_msg=f"set {k} scene {q}")
            assert np.array_equal(ptr_e[k, ROFF[q]: ROFF[q + 1]], ptr), (k, q)
            assert np.array_equal(zn_e[k, ROFF[q]: ROFF[q + 1]] != 0, zn != 0), (k, q)
    ref = _sums_reference(states, ds["obj"], FEAT, rc.LENGTHS, ROFF, K)
    _check_sums(sums, ref, rc.LENGTHS, ROFF, len(FEAT))
    print("largest twin difference per scene a - f:", " ".join(f"{w:.1e}" for w in worst))
    return float(worst.max())


@pytest.mark.parametrize("model,rule", CONFIGS)
def test_roaded_scenes_equal_their_twins(model, rule):
    """the six scenes of scene_road_common x 7 sets in one launch against 42 stand-alone engines with set_road on the one-wave tick;
    the per-rider sums against NumPy on the call's own states (relative 2 m 2^-53)"""
    ds = _dataset(model, rule)
    e = ds["engine"]
    sums, states = e.scene_calib_eval(ds["sets"], states=True)       # (the read-backs below show THIS evaluation)
    assert np.array_equal(sums, ds["road"][0]) and np.array_equal(states, ds["road"][1])
    assert np.isfinite(states).all() and np.isfinite(sums).all()
    worst = _against_twins(ds, model, sums, states)
    print(f"{model} rule {rule}: largest |scene_calib_eval with roads - csf_step twin with set_road| = {worst:.3e} (expected 0)")


@pytest.mark.parametrize("model,rule", CONFIGS)
def test_road_parameters_per_candidate_set(model, rule):
    """road_F0 / road_sigma per set - integer and fractional sigmas, one set with F0 = 0 - against twins given those values on every
    edge through set_road; the set with F0 = 0 equals the evaluation without roads"""
    ds = _dataset(model, rule)
    e = ds["engine"]
    f0, sg = np.array([o[0] for o in rc.OVERRIDES]), np.array([o[1] for o in rc.OVERRIDES])
    sums, states = e.scene_calib_eval(ds["sets"], states=True, road_F0=f0, road_sigma=sg)
    worst = _against_twins(ds, model, sums, states, over=rc.OVERRIDES)
    print(f"{model} rule {rule}: largest |road overrides - twin| = {worst:.3e} (expected 0)")
    R, z = ds["R"], rc.ZERO_SET
    e.scene_calib_road(None, None, None, None, None)
    s_bare, st_bare = e.scene_calib_eval(ds["sets"], states=True)
    e.scene_calib_road(*rc.road_args(model))
    assert np.array_equal(s_bare, ds["bare"][0]) and np.array_equal(st_bare, ds["bare"][1])
    assert np.array_equal(states[:, z * R: (z + 1) * R], st_bare[:, z * R: (z + 1) * R])
    assert np.array_equal(sums[z], s_bare[z])
    # the evaluation after an override is the plain one again
    again = e.scene_calib_eval(ds["sets"], states=True)
    assert np.array_equal(again[0], ds["road"][0]) and np.array_equal(again[1], ds["road"][1])


@pytest.mark.parametrize("model,rule", CONFIGS)
def test_the_road_acts(model, rule):
    """on the roaded scenes every rider of every set ends more than 1e-6 m from where it ends without roads (the CPU oracle gives
    100 x that: tests/test_scene_road_host.py); two sets that differ only in road_F0 give different sums"""
    ds = _dataset(model, rule)
    R, K = ds["R"], ds["K"]
    least = np.inf
    for q in range(len(rc.N_RIDERS)):
        last = int(rc.LENGTHS[q]) - 1
        for k in range(K):
            sl = slice(k * R + ROFF[q], k * R + ROFF[q + 1])
            d = np.hypot(ds["road"][1][last, sl, 0] - ds["bare"][1][last, sl, 0], ds["road"][1][last, sl, 1] - ds["bare"][1][last, sl, 1])
            if rc.ROADS[q] is None:
                assert np.all(d == 0.0), (q, k)
            else:
                least = min(least, float(d.min()))
                assert np.all(d > 1e-6), (q, k, d)
    print(f"{model} rule {rule}: the least a road moves a rider: {least:.3e} m")
    two = ds["engine"].scene_calib_eval([ds["sets"][0], ds["sets"][0]], road_F0=[4.0, 4.5], road_sigma=[2.0, 2.0])
    roaded = np.concatenate([np.arange(ROFF[q], ROFF[q + 1]) for q in range(len(rc.N_RIDERS)) if rc.ROADS[q] is not None])
    assert np.all(np.any(two[0, roaded] != two[1, roaded], axis=1))
    bare = np.concatenate([np.arange(ROFF[q], ROFF[q + 1]) for q in range(len(rc.N_RIDERS)) if rc.ROADS[q] is None])
    assert np.array_equal(two[0, bare], two[1, bare])


def test_dropping_the_roads_and_a_replay_on_a_roaded_scene():
    from cyclistsocialforce_amd.engine import Engine
    ds = _dataset("twod", 0)
    e, sets, R, K = ds["engine"], ds["sets"], ds["R"], ds["K"]
    s0, off, rows = ds["load"]
    e.scene_calib_road([], None, None, None, None)
    dropped = e.scene_calib_eval(sets, states=True)
    never = Engine(sets[0], K * R)
    never.scene_calib_load(rc.N_RIDERS, s0, VDES, off, rows, ds["obj"], FEAT, lengths=rc.LENGTHS, max_sets=K)
    fresh = never.scene_calib_eval(sets, states=True)
    never.close()
    assert np.array_equal(dropped[0], fresh[0]) and np.array_equal(dropped[1], fresh[1])
    with pytest.raises(Exception):
        e.scene_calib_eval(sets, road_F0=np.ones(K), road_sigma=np.full(K, 2.0))      # no scene has a road now
    # a replayed rider on a roaded scene: the first rider of scenes c, d and f follows what set 0 recorded for it
    e.scene_calib_road(*rc.road_args("twod"))
    mask = np.zeros(R, dtype=bool)
    mask[[ROFF[2], ROFF[3], ROFF[5]]] = True
    rec = np.ascontiguousarray(ds["road"][1][:, :R][:, mask, :4])
    e.scene_calib_replay(mask, rec)
    sums, states = e.scene_calib_eval(sets, states=True, road_F0=np.full(K, 7.0), road_sigma=np.full(K, 2.0))
    for q in (2, 3, 5):
        ln = int(rc.LENGTHS[q])
        for k in range(K):
            assert np.array_equal(states[:ln, k * R + ROFF[q], :4], ds["road"][1][:ln, ROFF[q], :4]), (q, k)
            assert np.all(sums[k, ROFF[q]] == 0.0)
    # ... and with the roads' own parameters set 0, whose recording it is, is what it was
    sums, states = e.scene_calib_eval(sets, states=True)
    sim = ~mask
    assert np.array_equal(states[:, :R][:, sim, :4], ds["road"][1][:, :R][:, sim, :4])
    e.scene_calib_replay(None)
    again = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(again[0], ds["road"][0]) and np.array_equal(again[1], ds["road"][1])


@pytest.mark.parametrize("case", rc.ORACLE_ROAD_CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_roaded_scenes_against_the_oracle(case):
    """one TwoD, one Bicycle and one PlanarPoint case of ORACLE_CASES between two road edges, the three oracle_fields sets in one
    launch, 200 ticks against orc.Population with set_road: positions at stride 10 within 1e-4 x extent.  The oracle's own
    sensitivity on these cases is held below 1e-5 x extent by tests/test_scene_road_host.py."""
    from cyclistsocialforce_amd.engine import Engine
    m, n, rule, hfov = case
    s0, off, dq, pods = oracle_case(m, n, rule, hfov)
    road = rc.oracle_road()
    e = Engine(pods[0], len(pods) * n)
    e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((rc.ORACLE_TICKS, n, 1)), [0], max_sets=len(pods))
    _, bare = e.scene_calib_eval(pods, states=True, stride=10)
    e.scene_calib_road(np.zeros(2, dtype=np.int32), *road)
    _, states = e.scene_calib_eval(pods, states=True, stride=10)
    e.close()
    for k, pod in enumerate(pods):
        ref = rc.oracle_road_run(pod, s0, off, dq, road, rc.ORACLE_TICKS)
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        got = states[:, k * n: (k + 1) * n, :2]
        worst = float(np.hypot(got[..., 0] - ref[..., 0], got[..., 1] - ref[..., 1]).max())
        moved = float(np.abs(got - bare[:, k * n: (k + 1) * n, :2]).max())
        print(f"{m} n={n} rule={rule} set {k}: largest position deviation {worst:.3e} m = {worst / ext:.2e} x extent; the road moves a rider by up to {moved:.3e} m")
        assert worst < 1e-4 * ext, (case, k)
        assert moved > 1e-4 * ext, (case, k)


def test_refusals_change_nothing():
    from cyclistsocialforce_amd import _ffi
    from cyclistsocialforce_amd.engine import Engine, EngineError
    ds = _dataset("twod", 0)
    e, sets, R, K = ds["engine"], ds["sets"], ds["R"], ds["K"]
    L, h = e._lib, e._h
    P = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    es, off, verts, f0, sg = rc.road_args("twod")
    tab = (_ffi.Params * K)(*sets)
    sums = np.zeros((K, R, 2))
    E_ARG, E_STATE = -1, -4

    def same():
        got = e.scene_calib_eval(sets, states=True)
        assert np.array_equal(got[0], ds["road"][0]) and np.array_equal(got[1], ds["road"][1])

    def road(code, what, n=None, es_=es, off_=off, verts_=verts, f0_=f0, sg_=sg):
        rcode = L.csf_scene_calib_road(h, (es.size if es_ is None else es_.size) if n is None else n, P(es_), P(off_), P(verts_), P(f0_), P(sg_))
        assert rcode == code and L.csf_last_error(h), (what, rcode)
        same()

    def ev(code, what, f0_, sg_):
        rcode = L.csf_scene_calib_eval_road(h, K, tab, C.sizeof(_ffi.Params), _ffi.ABI_VERSION, P(f0_), P(sg_), P(sums), 1, None)
        assert rcode == code and L.csf_last_error(h), (what, rcode)
        same()

    for name in ("es_", "off_", "verts_", "f0_", "sg_"):
        road(E_ARG, f"NULL {name}", **{name: None})
    road(E_ARG, "a negative number of edges", n=-1)
    bad = es.copy(); bad[-1] = len(rc.N_RIDERS)
    road(E_ARG, "a scene beyond the data set", es_=bad)
    bad = es.copy(); bad[0] = -1
    road(E_ARG, "a negative scene", es_=bad)
    bad = es.copy(); bad[1] = bad[2] + 1
    road(E_ARG, "decreasing edge_scene", es_=bad)
    bad = off.copy(); bad[2] = bad[1] - 1
    road(E_ARG, "offsets that run backwards", off_=bad)
    for arr, name in ((verts, "verts_"), (f0, "f0_"), (sg, "sg_")):
        for v in (np.nan, np.inf):
            bad = arr.copy(); bad.reshape(-1)[0] = v
            road(E_ARG, f"{v} in {name}", **{name: bad})
    xs = np.c_[np.linspace(-20.0, 50.0, 2049), np.full(2049, -3.0)]
    one = lambda q, nv: dict(es_=np.array([q], dtype=np.int32), off_=np.array([0, nv], dtype=np.int64), verts_=xs, f0_=np.ones(1), sg_=np.full(1, 2.0))  # noqa: E731
    road(E_ARG, "513 vertices on the scene of 32 riders", **one(4, 513))
    for q in (0, 2, 3):
        road(E_ARG, f"2 049 vertices on scene {q}", **one(q, 2049))
    one_f, one_s = np.full(K, 1.0), np.full(K, 2.0)
    ev(E_ARG, "road_F0 without road_sigma", one_f, None)
    ev(E_ARG, "road_sigma without road_F0", None, one_s)
    for v in (-0.5, np.nan, np.inf):
        bad = one_f.copy(); bad[3] = v
        ev(E_ARG, f"road_F0 = {v}", bad, one_s)
    for v in (np.nan, -np.inf):
        bad = one_s.copy(); bad[K - 1] = v
        ev(E_ARG, f"road_sigma = {v}", one_f, bad)
    # an override when no scene has a road; the road call without a closed-loop data set, and on the data set of csf_calib_load
    e.scene_calib_road(None, None, None, None, None)
    rcode = L.csf_scene_calib_eval_road(h, K, tab, C.sizeof(_ffi.Params), _ffi.ABI_VERSION, P(one_f), P(one_s), P(sums), 1, None)
    assert rcode == E_STATE and L.csf_last_error(h)
    got = e.scene_calib_eval(sets, states=True)
    assert np.array_equal(got[0], ds["bare"][0]) and np.array_equal(got[1], ds["bare"][1])
    e.scene_calib_road(es, off, verts, f0, sg)
    same()
    plain = Engine(sets[0], 8)
    assert L.csf_scene_calib_road(plain._h, es.size, P(es), P(off), P(verts), P(f0), P(sg)) == E_STATE and L.csf_last_error(plain._h)
    with pytest.raises(EngineError):
        plain.scene_calib_road(es, off, verts, f0, sg)
    F1 = np.zeros((1, 1))
    plain.calib_load(np.zeros((1, plain.ns)), F1, F1, np.zeros((1, 1, 1)), [0], max_sets=1)
    assert L.csf_scene_calib_road(plain._h, es.size, P(es), P(off), P(verts), P(f0), P(sg)) == E_STATE and L.csf_last_error(plain._h)
    plain.close()
    # csf_scene_calib_load still refuses an engine with a road of its own, and says where scene roads go
    own = Engine(sets[0], K * R)
    own.set_road([0, 2], [[0.0, 0.0], [10.0, 0.0]], [1.0], [1.0])
    s0, doff, rows = ds["load"]
    with pytest.raises(EngineError, match="csf_scene_calib_road"):
        own.scene_calib_load(rc.N_RIDERS, s0, VDES, doff, rows, ds["obj"], FEAT, lengths=rc.LENGTHS, max_sets=K)
    own.close()


def test_recovery_of_a_field_and_a_road_parameter():
    """8 roaded scenes of 3 - 5 TwoD riders x 60 ticks whose trajectories the engine itself produced with the default set and
    road_F_0 = 0.15; started 30 % off, fmin and run_many return (f_0, road_F_0) within xtol of the truth"""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    from cyclistsocialforce_amd.engine import Engine
    pod = parameters.default_pod("twod")
    star = np.array([pod.f_0, 0.15])
    data = []
    for q in range(len(rc.RECOVERY_N)):
        s0, off, dq, road = rc.recovery_scene(q)
        n = s0.shape[0]
        e = Engine(pod, n)
        e.scene_calib_load([n], s0, 5.0, off, dq, np.zeros((rc.RECOVERY_TICKS, n, 1)), [0], max_sets=1)
        e.scene_calib_road(np.zeros(2, dtype=np.int32), *road)
        _, st = e.scene_calib_eval([pod], states=True)
        e.close()
        data.append(cal.SceneData(s0, 5.0, off, dq, st, road=road))
    xtol = 1e-4
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, ["f_0", "road_F_0"], data, data, [1, 1, 0, 0, 0, 0], max_sets=8, maxiter=400,
                                   xtol=xtol, ftol=1e-30)
    f_star = c.evaluate([star])[0]
    guesses = [star * [1.3, 0.7], star * [0.7, 1.3]]
    f_start = c.evaluate(guesses)
    res = c.run(guesses[0])
    many = c.run_many(guesses)
    print("recovery: run", res[0], res[1], "iterations", res[2], "| run_many", [(x, f, it) for x, f, it in many], "| f(theta*)", f_star, "f(guesses)", f_start)
    assert f_star == 0.0
    assert np.abs(res[0] - star).max() <= xtol and res[1] < 1e-6 * f_start[0]
    for (x, f, it), f0 in zip(many, f_start):
        assert np.abs(x - star).max() <= xtol, (x, star)
        assert f < 1e-6 * f0
    c.close()


def test_the_abi_in_a_fresh_process():
    """the two entry points through raw ctypes in a process of its own; after csf_scene_calib_clear a small population takes the
    one-wave tick"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "scene_road_abi_child.py")], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here) + os.pathsep + here})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "scene road abi ok" in r.stdout

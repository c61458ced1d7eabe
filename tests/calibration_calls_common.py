"""Shared by tests/test_calibration_calls_host.py and tests/golden/make_golden_calibration_calls.py: the CALL TRANSCRIPT of
cyclistsocialforce_amd/calibration.py (the Python layering).  A recording engine stands in for `Engine` - passed as
`engine_factory` to InteractionCalibration, patched in place of `calibration.Engine` for DownhillSimplexCalibration - and logs every
constructor and method call in order: array-likes as (dtype, shape, SHA-256 of the bytes of np.ascontiguousarray), parameter records as
the digest of bytes(pod), everything else by repr.  What it returns is a fixed pseudo-random function of (pod bytes, road override,
rider index) - sums whose total depends on the order they are added in, states of the right shape with the same property - so the
returned errors, trajectories and downhill-simplex results pin the arithmetic of the host code as well.  No GPU, no library.

`transcripts()` runs every case and returns {case name: list of entries}; an entry is ["call", name, args, kwargs], ["value", label,
...] or ["raises", label, exception type, message, an engine had been made]."""
import hashlib

import numpy as np

from cyclistsocialforce_amd import _ffi, calibration as cal, vehicle

FEAT_XY = [1, 1, 0, 0, 0, 0]


# --------------------------------------------------------------------------- the recording engine
def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _holds_pod(x):
    return isinstance(x, _ffi.Params) or (isinstance(x, (list, tuple)) and any(_holds_pod(y) for y in x))


def described(x):
    """one argument as the transcript holds it"""
    if isinstance(x, _ffi.Params):
        return ["pod", _sha(bytes(x))]
    if _holds_pod(x):
        return ["seq", [described(y) for y in x]]
    if isinstance(x, (np.ndarray, list, tuple)):
        a = np.ascontiguousarray(x)
        if a.dtype != object:
            return ["array", str(a.dtype), list(a.shape), _sha(a.tobytes())]
    return ["repr", repr(x)]


def _rng(pods, k, road_F0, road_sigma):
    """the generator of candidate k: a function of its pod bytes and its road overrides"""
    tup = pods[k] if isinstance(pods[k], tuple) else (pods[k],)
    h = hashlib.sha256(b"".join(bytes(p) for p in tup))
    for over in (road_F0, road_sigma):
        h.update(b"-" if over is None else np.float64(over[k]).tobytes())
    return np.random.default_rng(int.from_bytes(h.digest()[:8], "little"))


class RecordingEngine:
    """every call of calibration.py on an engine, logged to `log` (a subclass per case carries the list)"""
    log = None

    def __init__(self, pod, capacity, device=0):
        self.ns = _ffi.N_STATES[pod.model]
        self._call("Engine", (pod, capacity), dict(device=device))

    def _call(self, name, args, kw):
        self.log.append(["call", name, [described(a) for a in args], {k: described(v) for k, v in sorted(kw.items())}])

    def _loaded(self, name, s0, table, args, kw):
        self.R, self.T = np.asarray(s0).shape[0], np.asarray(table).shape[0]
        self._call(name, args, kw)

    def calib_load(self, s0, Fx, *args, **kw):
        self._loaded("calib_load", s0, Fx, (s0, Fx) + args, kw)

    def scene_calib_load(self, nr, s0, vd, off, rows, obj, *args, **kw):
        self._loaded("scene_calib_load", s0, obj, (nr, s0, vd, off, rows, obj) + args, kw)

    def scene_calib_load_shared(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, *args, **kw):
        self._loaded("scene_calib_load_shared", s0, obj, (nr, nl, lane, enter, exit, s0, vd, off, rows, obj) + args, kw)

    def scene_calib_load_wide(self, nr, nl, lane, enter, exit, s0, vd, off, rows, obj, *args, **kw):
        self._loaded("scene_calib_load_wide", s0, obj, (nr, nl, lane, enter, exit, s0, vd, off, rows, obj) + args, kw)

    def scene_calib_classes(self, group, models=None, s0=None):
        self.ns = max(_ffi.N_STATES[m] for m in models)
        self._call("scene_calib_classes", (group, models, s0), {})

    def _evaluated(self, name, pods, args, kw):
        self._call(name, (pods,) + args, kw)
        stride, sums = kw.get("stride", 1), np.zeros((len(pods), self.R, 2))
        states = np.zeros((self.T // stride, len(pods) * self.R, self.ns))
        for k in range(len(pods)):
            rng = _rng(pods, k, kw.get("road_F0"), kw.get("road_sigma"))
            sums[k] = rng.uniform(0.1, 10.0, size=(self.R, 2))
            states[:, k * self.R: (k + 1) * self.R] = rng.normal(size=(self.T // stride, self.R, self.ns))
        return (sums, states) if kw.get("states") else sums

    def calib_eval(self, pods, *args, **kw):
        return self._evaluated("calib_eval", pods, args, kw)

    def scene_calib_eval(self, pods, *args, **kw):
        return self._evaluated("scene_calib_eval", pods, args, kw)

    def scene_calib_eval_groups(self, pods, *args, **kw):
        return self._evaluated("scene_calib_eval_groups", pods, args, kw)


def _logged(name):
    def method(self, *args, **kw):
        self._call(name, args, kw)
    method.__name__ = name
    return method


for _name in ("scene_calib_groups", "scene_calib_lane_groups", "scene_calib_replay", "scene_calib_road", "scene_calib_windows", "close"):
    setattr(RecordingEngine, _name, _logged(_name))


def engine_class(log):
    return type("CaseEngine", (RecordingEngine,), dict(log=log))


# --------------------------------------------------------------------------- what a case writes down
def hexes(values):
    return [float(v).hex() for v in np.asarray(values, dtype=float).ravel()]


def _value(log, label, *what):
    log.append(["value", label] + list(what))


def _refusal(log, label, fn):
    """fn() must raise: the exception type, its full message and whether an engine had been made by then"""
    at = len(log)
    try:
        fn()
    except Exception as exc:                                      # noqa: BLE001  (the type is what is recorded)
        made = any(e[0] == "call" and e[1] == "Engine" for e in log[at:])
        log.append(["raises", label, type(exc).__name__, str(exc), made])
        return
    raise AssertionError(f"{label}: nothing was raised")


def custom_error(outputs, objectives):
    """an error function that is neither of the built-in two: order-dependent, and blind to the NaN outside a presence window"""
    return sum(float(np.nansum(np.abs(np.asarray(o) - np.asarray(b)) ** 1.5)) for o, b in zip(outputs, objectives))


def _optimum(c):
    return [[repr(k), float(v).hex()] for k, v in c.param_args_opt.items()]


# --------------------------------------------------------------------------- scenes
def scene(seed, n, ticks, cols=4, width=5, queue=2, **kw):
    """a scene of plain random arrays: n road users, `ticks` recorded rows, 1 .. `queue` destination rows each"""
    rng = np.random.default_rng(seed)
    off = np.r_[0, np.cumsum(rng.integers(1, queue + 1, size=n))]
    return cal.SceneData(rng.normal(size=(n, width)), rng.uniform(4.0, 6.0, size=n), off, rng.normal(size=(off[-1], 3)),
                         rng.normal(size=(ticks, n, cols)), **kw)


ROAD = ([0, 3, 5], [[0.0, -3.0], [5.0, -3.0], [9.0, -2.5], [0.0, 4.0], [9.0, 4.5], [99.0, 99.0]], [6.0, 5.0], [2.0, 2.5])


def _plain():
    return [scene(1, 3, 12, length=9), scene(2, 2, 8), scene(3, 2, 5, length=0)]


def _replay():
    rng = np.random.default_rng(4)                                # rider 1 follows its recording and has no queue of its own
    first = cal.SceneData(rng.normal(size=(3, 5)), 5.0, [0, 2, 2, 3], rng.normal(size=(3, 3)), rng.normal(size=(10, 3, 4)),
                          replayed=[False, True, False])
    return [first] + scene(5, 3, 12, length=11).ego_split()


def _roads():
    return [scene(6, 3, 10, road=ROAD), scene(7, 2, 12)]


def _windows():
    rng = np.random.default_rng(8)
    enter, exit_ = np.array([0, 3, 5, 2]), np.array([12, 3, 10, 9])   # rider 1: never present; rider 3: replayed, window interior
    traj = rng.normal(size=(12, 4, 4))
    traj[:5, 2] = traj[10:, 2] = np.nan                           # (outside a window the recording is never read)
    traj[:2, 3] = traj[9:, 3] = np.nan
    return [cal.SceneData(rng.normal(size=(4, 5)), 5.0, np.arange(5), rng.normal(size=(4, 3)), traj, replayed=[False, False, False, True],
                          present=(enter, exit_)), scene(9, 2, 8)]


def _roster34(**kw):
    return scene(10, 34, 40, queue=1, present=(np.arange(34), np.arange(34) + 3), **kw)


def _wide40(**kw):
    return scene(11, 40, 10, queue=1, wide=True, **kw)


def _grouped(d, group):
    """the scene d with its road users in groups"""
    return cal.SceneData(d.s0, d.v_desired, d.dest_offsets, d.dest_xyz_stop, d.traj, length=d.length, replayed=d.replayed, road=d.road,
                         present=(d.enter, d.exit) if d.windowed or d.n > 32 else None, wide=d.wide, group=group)


def _groups(data):
    return [_grouped(d, np.arange(d.n) % 2) for d in data]


def _mixed():
    return [_grouped(scene(12, 3, 10, width=5), [0, 1, 0]), _grouped(scene(13, 4, 8, width=8, cols=6), [1, 1, 0, 0])]


GROUP_KEYS = [("f_0", 0), ("f_0", 1), "sigma_0"]
GP = [dict(hfov=2.0), dict(hfov=3.0, e_0=0.9)]
TWO = [vehicle.TwoDBicycle, vehicle.InvPendulumBicycle]

# name -> (vehicle_type, params_keys, the vector the candidates are spread around, scenes, keyword arguments)
INTERACTION = {
    "plain": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], _plain, {}),
    "replay": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], _replay, {}),
    "road_F_0": (vehicle.TwoDBicycle, ["f_0", "road_F_0"], [7.0, 0.05], _roads, {}),
    "road_both": (vehicle.TwoDBicycle, ["road_sigma", "f_0", "road_F_0"], [3.0, 7.0, 0.05], _roads, {}),
    "windows": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], _windows, {}),
    "shared_roster": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], lambda: [_roster34(), scene(14, 3, 10)], {}),
    "shared_asked": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], lambda: [scene(15, 3, 10), scene(16, 2, 12, length=7)], dict(share_lanes=True)),
    "wide_33": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], lambda: [_wide40(), scene(17, 3, 12)], {}),
    "wide_2": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], lambda: [_wide40(), scene(17, 3, 12)], dict(wide_from=2)),
    "wide_33_road": (vehicle.TwoDBicycle, ["f_0", "road_F_0"], [7.0, 0.05], lambda: [_wide40(road=ROAD), scene(17, 3, 12)], {}),
    "wide_2_road": (vehicle.TwoDBicycle, ["f_0", "road_F_0"], [7.0, 0.05], lambda: [_wide40(road=ROAD), scene(17, 3, 12, road=ROAD)], dict(wide_from=2)),
    "groups_plain": (vehicle.TwoDBicycle, GROUP_KEYS, [7.0, 9.0, 0.5], lambda: _groups(_plain()), dict(group_params=GP)),
    "groups_shared": (vehicle.TwoDBicycle, GROUP_KEYS, [7.0, 9.0, 0.5], lambda: _groups([_roster34(), scene(14, 3, 10)]),
                      dict(group_params=GP, lane_groups=True)),
    "groups_wide": (vehicle.TwoDBicycle, GROUP_KEYS, [7.0, 9.0, 0.5], lambda: _groups([_wide40(), scene(17, 3, 12)]),
                    dict(group_params=GP, lane_groups=True)),
    "one_group": (vehicle.TwoDBicycle, ["f_0", "sigma_0"], [7.0, 0.5], _plain, dict(group_params=[dict(hfov=2.0)])),
    "mixed": (TWO, GROUP_KEYS, [7.0, 9.0, 0.5], _mixed, {}),
}


def _spread(base, k):
    return np.asarray(base, dtype=float)[None, :] * (1.0 + 0.07 * np.arange(k))[:, None]


def interaction_case(name):
    """all three error functions on five vectors in chunks of two; with the first: test() before a run, simulate, run_many, test() after
    it, and the empty test data"""
    log = []
    E = engine_class(log)
    vtype, keys, base, make, kw = INTERACTION[name]
    data = make()
    vectors = _spread(base, 5)
    for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples, custom_error):
        c = cal.InteractionCalibration(vtype, keys, data, data[::-1], FEAT_XY, error_func=func, max_sets=2, maxiter=3, engine_factory=E, **kw)
        _value(log, "evaluate " + func.__name__, hexes(c.evaluate(vectors)))
        if func is cal.calc_sse_timesteps:
            _refusal(log, "test before a run", c.test)
            trajs, objs = c.simulate(vectors[1])
            _value(log, "simulate", [described(t) for t in trajs], [described(o) for o in objs])
            _value(log, "test of a vector", float(c.test(vectors[2])).hex())
            res = c.run_many(list(vectors[:2] * 1.01))
            _value(log, "run_many", [[hexes(x), float(f).hex(), int(it)] for x, f, it in res], _optimum(c))
            _value(log, "test after the run", float(c.test()).hex())
        c.close()
    c = cal.InteractionCalibration(vtype, keys, data, [], FEAT_XY, max_sets=2, engine_factory=E, **kw)
    _refusal(log, "no test scenes", lambda: c.test(vectors[0]))
    return log


# --------------------------------------------------------------------------- DownhillSimplexCalibration
def _samples(seed=20):
    rng = np.random.default_rng(seed)
    keys = ["Fx", "Fy", "x", "y", "psi", "v", "delta", "theta"]
    return cal.CalibrationData([rng.normal(size=(n, 8)) for n in (8, 5, 11)], [0, 0, 1, 0, 1, 1, 0, 1], [1, 1, 0, 0, 0, 0, 0, 0], feature_keys=keys)


def _scaled(v, s=1.0):
    return s * v[0]


def _summed(v):
    return 0.5 * (v[0] + v[1])


def simplex_case(aux):
    """three samples of unequal length, an objective row (theta) the Bicycle lacks; evaluate, simulate_single both ways, test, run_many"""
    log = []
    E, held = engine_class(log), cal.Engine
    kw = dict(params_auxfuncs=[_scaled, _summed], params_auxfuncsargs=[dict(s=1.1), {}]) if aux else {}
    data, feat = _samples(), [1, 0, 1, 1, 0, 1]
    vectors = _spread([10.0, 9.0], 5)
    cal.Engine = E
    try:
        for func in (cal.calc_sse_timesteps, cal.calc_maesse_samples, custom_error):
            c = cal.DownhillSimplexCalibration(vehicle.Bicycle, ["k_p_v", "k_p_delta"], data, _samples(21), feat, error_func=func, maxiter=3,
                                               verbose=False, max_sets=2, fix_speed=func is not custom_error, **kw)
            _value(log, "evaluate " + func.__name__, hexes(c.evaluate(vectors)), hexes(c.evaluate(vectors[:3], test=True)))
            if func is cal.calc_sse_timesteps:
                _refusal(log, "test before a run", c.test)
                _refusal(log, "plotting", lambda: c.test(plot_results=True))
                args = c._update_params_args_dict(vectors[1])
                _value(log, "params_args", [[k, float(v).hex()] for k, v in args.items()])
                trajs, objs = c.simulate_single(args)
                _value(log, "simulate_single", [described(t) for t in trajs], [described(o) for o in objs])
                cars, objs = c.simulate_single(args, return_vehicles=True, test=True)
                _value(log, "vehicles", [[described(v.traj), int(v.i), hexes(v.s), v.id] for v in cars], [described(o) for o in objs])
                err, cars = c.test(args)
                _value(log, "test of a set", float(err).hex(), [described(v.traj) for v in cars])
                res = c.run_many(list(vectors[:2] * 1.01))
                _value(log, "run_many", [[hexes(x), float(f).hex(), int(it)] for x, f, it in res], _optimum(c))
                _value(log, "test after the run", float(c.test()[0]).hex())
            c.close()
    finally:
        cal.Engine = held
    return log


# --------------------------------------------------------------------------- refusals
def _sd(s0=None, v=5.0, off=None, rows=None, traj=None, n=3, ticks=6, **kw):
    """SceneData of n road users with one argument at a time replaced by a faulty one"""
    rng = np.random.default_rng(30)
    return cal.SceneData(rng.normal(size=(n, 5)) if s0 is None else s0, v, np.arange(n + 1) if off is None else off,
                         rng.normal(size=(n, 3)) if rows is None else rows, rng.normal(size=(ticks, n, 4)) if traj is None else traj, **kw)


def _nan_traj(n=3, ticks=6, at=(2, 1, 0)):
    t = np.random.default_rng(31).normal(size=(ticks, n, 4))
    t[at] = np.nan
    return t


def _ic(E, keys=("f_0",), train=None, test=None, vtype=vehicle.TwoDBicycle, feat=FEAT_XY, **kw):
    train = [scene(40, 3, 6)] if train is None else train
    return cal.InteractionCalibration(vtype, list(keys), train, train if test is None else test, feat, max_sets=2, engine_factory=E, **kw)


def _loaded(E, **kw):
    return _ic(E, **kw).evaluate([[7.0]] if len(kw.get("keys", ("f_0",))) == 1 else [[7.0, 9.0]])


def _dsc(E, data):
    held, cal.Engine = cal.Engine, E
    try:
        return cal.DownhillSimplexCalibration(vehicle.Bicycle, ["k_p_v"], data, data, FEAT_XY, verbose=False).evaluate([[10.0]])
    finally:
        cal.Engine = held


def _finished_run():
    run = cal.NelderMead([1.0, 2.0], maxiter=0)
    run.tell([3.0, 2.0, 1.0])
    run.tell([1.0])


def _past_the_end():
    it = iter(_samples())
    for _ in range(4):
        next(it)


EDGES_300 =([0, 300], np.c_[np.arange(300.0), np.zeros(300)], 1.0, 1.0)

# label -> a call that raises; E is the case's engine class.  The comment names the `raise` of calibration.py it reaches.
REFUSALS = {
    # ---- helpers, data, downhill simplex
    "indicators: shape": lambda E: cal.CalibrationData([np.zeros((3, 6))], [1, 0], [1, 1, 0, 0, 0, 0], feature_keys=list("abcdef")),
    "indicators: values": lambda E: cal.CalibrationData([np.zeros((3, 6))], [2, 0, 0, 0, 0, 0], [1, 1, 0, 0, 0, 0], feature_keys=list("abcdef")),
    "track: keys": lambda E: cal.Track(np.zeros((3, 6)), ["a", "b"]),
    "data: no tracks": lambda E: cal.CalibrationData([], [1], [1]),
    "data: features differ": lambda E: cal.CalibrationData([cal.Track(np.zeros((3, 2)), "ab"), cal.Track(np.zeros((3, 3)), "abc")], [1, 0], [0, 1]),
    "data: iteration ends": lambda E: _past_the_end(),
    "partition: shares": lambda E: _samples().partition(2, [0.7, 0.7]),
    "simplex: maxiter": lambda E: cal.NelderMead([1.0, 2.0]),
    "simplex: tell when done": lambda E: _finished_run(),
    "dsc: auxfuncsargs alone": lambda E: cal.DownhillSimplexCalibration(None, ["a"], None, None, FEAT_XY, params_auxfuncsargs=[{}]),
    "dsc: auxfuncs count": lambda E: cal.DownhillSimplexCalibration(None, ["a", "b"], None, None, FEAT_XY, params_auxfuncs=[abs]),
    "dsc: objective shape": lambda E: _dsc(E, _samples()),
    # ---- SceneData
    "scene: wide roster": lambda E: _sd(n=257, wide=True),
    "scene: roster": lambda E: _sd(n=33),
    "scene: s0 columns": lambda E: _sd(s0=np.zeros((3, 3))),
    "scene: v_desired": lambda E: _sd(v=[5.0, 5.0]),
    "scene: group shape": lambda E: _sd(group=[0, 1]),
    "scene: group kind": lambda E: _sd(group=[0.0, 1.0, 0.0]),
    "scene: group sign": lambda E: _sd(group=[0, -1, 0]),
    "scene: replayed": lambda E: _sd(replayed=[True, False]),
    "scene: offsets": lambda E: _sd(off=[0, 1, 1, 3]),
    "scene: offsets end": lambda E: _sd(off=[0, 1, 2, 4]),
    "scene: traj": lambda E: _sd(traj=np.zeros((6, 2, 4))),
    "scene: traj columns": lambda E: _sd(traj=np.zeros((6, 3, 7))),
    "scene: length": lambda E: _sd(length=7),
    "scene: present pair": lambda E: _sd(present=5),
    "scene: present kind": lambda E: _sd(present=(np.zeros(3), np.ones(3))),
    "scene: present shape": lambda E: _sd(present=(np.zeros(2, dtype=int), np.ones(3, dtype=int))),
    "scene: present range": lambda E: _sd(present=([0, 3, 0], [6, 2, 6])),
    "scene: present past length": lambda E: _sd(present=([0, 0, 0], [6, 7, 6])),
    "scene: peak": lambda E: _sd(n=34, present=(np.zeros(34, dtype=int), np.full(34, 6))),
    "scene: wide peak": lambda E: _sd(n=258, wide=True, present=(np.zeros(258, dtype=int), np.r_[np.full(257, 4), 0])),
    "scene: replay columns": lambda E: _sd(traj=np.zeros((6, 3, 3)), replayed=[True, False, False]),
    "scene: replay finite": lambda E: _sd(traj=_nan_traj(), replayed=[False, True, False]),
    "scene: replay finite in its window": lambda E: _sd(traj=_nan_traj(), replayed=[False, True, False], present=([0, 1, 0], [6, 4, 6])),
    "road: tuple": lambda E: _sd(road=(1, 2)),
    "road: offsets": lambda E: _sd(road=([0, 3, 2], np.zeros((3, 2)), 1.0, 1.0)),
    "road: offsets past the vertices": lambda E: _sd(road=([0, 4], np.zeros((3, 2)), 1.0, 1.0)),
    "road: F0 count": lambda E: _sd(road=([0, 2, 3], np.zeros((3, 2)), [1.0, 2.0, 3.0], 1.0)),
    "road: finite": lambda E: _sd(road=([0, 2], [[0.0, 0.0], [np.inf, 0.0]], 1.0, 1.0)),
    "road: vertices": lambda E: _sd(n=32, road=([0, 2049], np.zeros((2049, 2)), 1.0, 1.0)),
    "road: vertices per power of two": lambda E: _sd(n=17, road=([0, 600], np.zeros((600, 2)), 1.0, 1.0)),
    "road: vertices of a wide scene": lambda E: _sd(n=3, wide=True, road=EDGES_300),
    "road: vertices on lanes": lambda E: _sd(n=34, ticks=40, present=(np.arange(34), np.arange(34) + 3), road=([0, 2049], np.zeros((2049, 2)), 1.0, 1.0)),
    # ---- InteractionCalibration: the constructor
    "types: count": lambda E: _ic(E, vtype=[vehicle.TwoDBicycle]),
    "types: not simulated": lambda E: _ic(E, vtype=[vehicle.TwoDBicycle, vehicle.UncontrolledVehicle]),
    "types: no vehicle class": lambda E: _ic(E, vtype=[vehicle.TwoDBicycle, "bicycle"]),
    "types: group_params count": lambda E: _ic(E, vtype=TWO, group_params=[{}]),
    "group_params: count": lambda E: _ic(E, group_params=[{}] * 5),
    "group_params: none": lambda E: _ic(E, group_params=[]),
    "keys: grammar": lambda E: _ic(E, keys=[("f_0", "a")], group_params=GP),
    "keys: a bool is no group": lambda E: _ic(E, keys=[("f_0", True)], group_params=GP),
    "keys: a list is no key": lambda E: _ic(E, keys=[["f_0", 0]], group_params=GP),
    "keys: road key per group": lambda E: _ic(E, keys=[("road_F_0", 0)], group_params=GP),
    "keys: group without group_params": lambda E: _ic(E, keys=[("f_0", 0)]),
    "keys: group out of range": lambda E: _ic(E, keys=[("f_0", 2)], group_params=GP),
    "keys: no parameter of a class": lambda E: _ic(E, keys=["f_0", "poles"], vtype=[vehicle.TwoDBicycle, vehicle.PlanarBicycle]),
    "keys: no parameter of its class": lambda E: _ic(E, keys=[("poles", 0)], vtype=[vehicle.TwoDBicycle, vehicle.PlanarBicycle]),
    "wide_from": lambda E: _ic(E, wide_from=258),
    "data: not a scene": lambda E: _ic(E, train=[scene(40, 3, 6), "scene"]),
    "data: group out of range": lambda E: _ic(E, test=[scene(40, 3, 6), _grouped(scene(41, 3, 6), [0, 1, 0])]),
    "data: group out of range of two": lambda E: _ic(E, train=[_grouped(scene(41, 3, 6), [0, 2, 0])], group_params=GP),
    "data: nothing to train on": lambda E: _ic(E, train=[], test=[scene(40, 3, 6)]),
    "features: shape": lambda E: _ic(E, feat=[1, 1, 0]),
    "features: none": lambda E: _ic(E, feat=[0] * 6),
    "road key: no road in train_data": lambda E: _ic(E, keys=["road_F_0"]),
    "road key: no road in test_data": lambda E: _ic(E, keys=["road_sigma"], train=[scene(6, 3, 10, road=ROAD)], test=[scene(40, 3, 6)]),
    "road key: an empty road is none": lambda E: _ic(E, keys=["road_F_0"], train=[scene(6, 3, 10, road=([0], np.zeros((0, 2)), [], []))]),
    # ---- InteractionCalibration: loading, evaluating, testing
    "pods: no parameter of a class": lambda E: _loaded(E, vtype=TWO, group_params=[{}, dict(bogus=1.0)], train=_mixed()),
    "load: all replayed": lambda E: _loaded(E, train=[scene(40, 3, 6), scene(42, 2, 6, replayed=[True, True])]),
    "load: nobody simulated is present": lambda E: _loaded(E, train=[scene(43, 2, 6, replayed=[True, False], present=([0, 3], [6, 3]))]),
    "load: objective row": lambda E: _loaded(E, train=[scene(40, 3, 6), scene(44, 3, 6, cols=1)]),
    "load: mixed classes on shared lanes": lambda E: _loaded(E, vtype=TWO, train=_mixed(), share_lanes=True),
    "load: mixed classes and a wide scene": lambda E: _loaded(E, vtype=TWO, train=_mixed() + [_grouped(_wide40(), np.arange(40) % 2)]),
    "load: groups on shared lanes": lambda E: _loaded(E, keys=GROUP_KEYS[:2], group_params=GP, train=_groups([_roster34()])),
    "load: groups and a wide scene": lambda E: _loaded(E, keys=GROUP_KEYS[:2], group_params=GP, train=_groups([_wide40()])),
    "load: groups, lanes asked for": lambda E: _loaded(E, keys=GROUP_KEYS[:2], group_params=GP, train=_groups(_plain()), share_lanes=True),
    # ---- two faults at once: which one is named
    "both: roster and v_desired": lambda E: _sd(n=33, v=[1.0, 2.0]),
    "both: group and window": lambda E: _sd(group=[0, -1, 0], present=([0, 3, 0], [6, 2, 6])),
    "both: window and road": lambda E: _sd(present=([0, 3, 0], [6, 2, 6]), road=(1, 2)),
    "both: replayed and offsets": lambda E: _sd(replayed=[True, False], off=[0, 1, 1, 3]),
    "both: traj and length": lambda E: _sd(traj=np.zeros((6, 2, 4)), length=9),
    "both: peak and replay": lambda E: _sd(n=34, traj=_nan_traj(34), replayed=np.arange(34) == 1, present=(np.zeros(34, dtype=int), np.full(34, 6))),
    "both: key and scene": lambda E: _ic(E, keys=[("f_0", 5)], group_params=GP, train=[scene(40, 3, 6), "scene"]),
    "both: types and key": lambda E: _ic(E, vtype=[vehicle.TwoDBicycle], keys=[("f_0", "a")]),
    "both: key grammar before class membership": lambda E: _ic(E, keys=["poles", ("f_0", 7)], vtype=[vehicle.TwoDBicycle, vehicle.PlanarBicycle]),
    "both: wide_from and scene": lambda E: _ic(E, wide_from=0, train=["scene"]),
    "both: group and no training scene": lambda E: _ic(E, train=[], test=[_grouped(scene(41, 3, 6), [0, 1, 0])]),
    "both: features and road key": lambda E: _ic(E, keys=["road_F_0"], feat=[0] * 6),
    "both: replayed scene before objective row": lambda E: _loaded(E, train=[scene(44, 3, 6, cols=1), scene(42, 2, 6, replayed=[True, True])]),
    "both: objective row before shared lanes": lambda E: _loaded(E, vtype=TWO, train=_mixed(), share_lanes=True, feat=[0, 0, 0, 0, 0, 1]),
    "both: mixed classes before groups": lambda E: _loaded(E, vtype=TWO, train=_mixed(), share_lanes=True, lane_groups=False),
}


def refusal_case():
    log = []
    E = engine_class(log)
    for label, fn in REFUSALS.items():
        _refusal(log, label, lambda: fn(E))
    return log


def transcripts():
    out = {"interaction " + name: interaction_case(name) for name in INTERACTION}
    out["simplex"] = simplex_case(False)
    out["simplex auxfuncs"] = simplex_case(True)
    out["refusals"] = refusal_case()
    return out

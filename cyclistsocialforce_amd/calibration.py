"""Calibration of rider-model parameters against recorded trajectories (the reference's calibration.py).

The names and signatures are the reference's: `calc_sse_timesteps`, `calc_maesse_samples`, `CalibrationData`,
`DownhillSimplexCalibration` (constructor, `_update_params_args_dict`, `simulate_single`, `run`, `test`, `param_args_opt`).
What differs is where the work is done: the data set is loaded onto the device once (`Engine.calib_load`), and an evaluation of
the objective is one kernel launch for ALL sequences and up to 256 candidate parameter sets (`Engine.calib_eval`); with one of the
two error functions above the error is summed on the device, so no trajectory is copied back.  On top of the reference's
interface: `evaluate` (many parameter vectors -> their errors, one launch) and `run_many` (independent downhill-simplex runs in
lockstep, every iteration of all of them one launch).

Two things are not the reference's:
  * a simulated sample is the state AFTER each tick, compared with the objective row of that tick (what the reference's `test`
    extracts: traj[:, 1 : i + 1]); the reference's `simulate_single` returns traj[:, :n], which leads with the start state;
  * `CalibrationData` is built from plain arrays (the reference's builds on the `trajdatamanager` package).
"""
from types import SimpleNamespace as _Namespace

import numpy as np

from . import _ffi
from .engine import Engine
from .parameters import RoadElementParameters

TRAJ_ROWS = 6  # rows of vehicle.traj an objective can name: x, y, psi, v, delta, theta (calibration.py:352-357)


# --------------------------------------------------------------------------- error functions
def calc_sse_timesteps(outputs, objectives):
    """Sum of squared errors over all time steps of all samples (calibration.py:27-50)."""
    return sum(float(np.square(np.asarray(out) - np.asarray(obj)).sum()) for out, obj in zip(outputs, objectives))


def calc_maesse_samples(outputs, objectives):
    """Sum over the samples of the squared mean absolute error of each (calibration.py:53-77)."""
    per_sample = [np.abs(np.asarray(out) - np.asarray(obj)).mean() for out, obj in zip(outputs, objectives)]
    return float(np.square(per_sample).sum()) if per_sample else 0


def objective_function_wrapper(params_vals, calibration):
    """The objective with the signature scipy's optimisers want (calibration.py:80-105)."""
    return float(calibration.evaluate(np.asarray(params_vals, dtype=float)[None, :])[0])


def _indicators(ind, name, n):
    """boolean indicator array of length n from booleans or 0 / 1 integers (utils.validate_boolean_indicators)"""
    a = np.asarray(ind)
    if a.shape != (n,):
        raise ValueError(f"{name} must have {n} entries, one per feature (got shape {a.shape})")
    if a.dtype != bool:
        if not np.all((a == 0) | (a == 1)):
            raise ValueError(f"{name} must hold booleans or 0 / 1")
        a = a.astype(bool)
    return a


# --------------------------------------------------------------------------- data
class Track:
    """One time series: data [n_t, n_features] and the keys of its columns; track["x"] is a column."""

    def __init__(self, data, data_feature_keys):
        self.data = np.asarray(data, dtype=float)
        self.data_feature_keys = list(data_feature_keys)
        if self.data.ndim != 2 or self.data.shape[1] != len(self.data_feature_keys):
            raise ValueError("a track is [n_t, n_features] with one key per feature")

    def __getitem__(self, key):
        return self.data[:, self.data_feature_keys.index(key)]


class CalibrationData:
    """A collection of tracks, each one sample of the data set (calibration.py:111-240).

    tracks: a list of [n_t, n_features] arrays (then `feature_keys` names their columns) or of Track objects.  Iterating yields
    (s0, input_data, objective_data) per track as calibration.py:165-208: the start state (x, y, psi, v, delta, theta - the last two
    0 where the tracks lack them) and rows 1 .. of the input and objective columns."""

    def __init__(self, tracks, objective_features, input_features, feature_keys=None):
        self.tracks = [t if isinstance(t, Track) else Track(t, feature_keys if feature_keys is not None else ()) for t in tracks]
        if not self.tracks:
            raise ValueError("no tracks")
        nf = self.tracks[0].data.shape[1]
        if any(t.data.shape[1] != nf for t in self.tracks):
            raise ValueError("the tracks of a data set share their features")
        self.objective_features = _indicators(objective_features, "objective_features", nf)
        self.input_features = _indicators(input_features, "input_features", nf)

    def __len__(self):
        return len(self.tracks)

    def __iter__(self):
        self._i_iter = 0
        return self

    def __next__(self):
        if self._i_iter >= len(self.tracks):
            raise StopIteration
        trk = self.tracks[self._i_iter]
        self._i_iter += 1
        s0 = np.zeros(TRAJ_ROWS)
        for k, key in enumerate(("x", "y", "psi", "v")):
            s0[k] = trk[key][0]
        if "delta" in trk.data_feature_keys:
            s0[4] = trk["delta"][0]
        if "theta" in trk.data_feature_keys:
            s0[5] = trk["theta"][0]
        return s0, trk.data[1:, self.input_features], trk.data[1:, self.objective_features]

    def partition(self, n_seq, shares, random_seed=None):
        """n_seq random subsets holding the given shares of the tracks (a seeded NumPy permutation; the last takes the rest)."""
        shares = np.asarray(shares, dtype=float)
        if shares.shape != (n_seq,) or abs(shares.sum() - 1.0) > 1e-9 or np.any(shares < 0):
            raise ValueError("shares: n_seq non-negative numbers that sum to 1")
        n = len(self.tracks)
        perm = np.random.default_rng(random_seed).permutation(n)
        cuts = np.floor(np.cumsum(shares)[:-1] * n + 1e-9).astype(int)
        return [CalibrationData([self.tracks[i] for i in part], self.objective_features, self.input_features)
                for part in np.split(perm, cuts)]


# --------------------------------------------------------------------------- downhill simplex, ask / tell
class NelderMead:
    """scipy.optimize.fmin's downhill simplex (Nelder and Mead 1965) turned inside out: `ask()` names the points whose values the
    next decision needs, `tell(values)` takes them.  Rules, arithmetic and order of operations are fmin's - initial simplex 5 % /
    0.00025, reflection 1, expansion 2, contraction 0.5, shrink 0.5, xtol = ftol = 1e-4 - so the simplices are the same to the
    last bit.  An iteration asks for reflection, expansion and both contractions at once (one launch for the caller) and uses
    what the rule needs; a shrink asks once more.  `maxiter` must be given: fmin then limits no function calls, and neither does this
    class (without it fmin also caps the CALLS at 200 per parameter, counted along its own sequence of evaluations - not restated)."""

    def __init__(self, x0, xtol=1e-4, ftol=1e-4, maxiter=None):
        if maxiter is None:
            raise ValueError("NelderMead: maxiter must be given (see the class docstring)")
        x0 = np.atleast_1d(np.asarray(x0, dtype=float)).flatten()
        self.N = N = len(x0)
        self.xtol, self.ftol = xtol, ftol
        self.maxiter = maxiter
        sim = np.empty((N + 1, N), dtype=x0.dtype)
        sim[0] = x0
        for k in range(N):
            y = np.array(x0, copy=True)
            y[k] = (1 + 0.05) * y[k] if y[k] != 0 else 0.00025
            sim[k + 1] = y
        self.sim = sim
        self.fsim = np.full((N + 1,), np.inf, dtype=float)
        self.iterations = 0
        self.state = "init"

    @property
    def done(self):
        return self.state == "done"

    @property
    def x(self):
        return self.sim[0]

    @property
    def fun(self):
        return np.min(self.fsim)

    def _sort(self):
        ind = np.argsort(self.fsim)
        self.sim = np.take(self.sim, ind, 0)
        self.fsim = np.take(self.fsim, ind, 0)

    def _next(self):
        sim, fsim = self.sim, self.fsim
        if not self.iterations < self.maxiter or (np.max(np.ravel(np.abs(sim[1:] - sim[0]))) <= self.xtol
                                                 and np.max(np.abs(fsim[0] - fsim[1:])) <= self.ftol):
            self.state = "done"
            return
        rho, chi, psi = 1, 2, 0.5
        xbar = np.add.reduce(sim[:-1], 0) / self.N
        self._cand = np.array([(1 + rho) * xbar - rho * sim[-1], (1 + rho * chi) * xbar - rho * chi * sim[-1],
                               (1 + psi * rho) * xbar - psi * rho * sim[-1], (1 - psi) * xbar + psi * sim[-1]])
        self.state = "iter"

    def ask(self):
        if self.state == "init":
            return self.sim.copy()
        if self.state == "iter":
            return self._cand.copy()
        if self.state == "shrink":
            return self.sim[1:].copy()
        return np.empty((0, self.N))

    def tell(self, f):
        f = np.asarray(f, dtype=float)
        sim, fsim = self.sim, self.fsim
        if self.state == "init":
            fsim[:] = f
            self._sort()
            self._sort()
            self.iterations = 1
            self._next()
            return
        if self.state == "shrink":
            fsim[1:] = f
        elif self.state == "iter":
            (xr, xe, xc, xcc), (fxr, fxe, fxc, fxcc) = self._cand, f
            doshrink = False
            if fxr < fsim[0]:
                if fxe < fxr:
                    sim[-1], fsim[-1] = xe, fxe
                else:
                    sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-2]:
                sim[-1], fsim[-1] = xr, fxr
            elif fxr < fsim[-1]:
                if fxc <= fxr:
                    sim[-1], fsim[-1] = xc, fxc
                else:
                    doshrink = True
            else:
                if fxcc < fsim[-1]:
                    sim[-1], fsim[-1] = xcc, fxcc
                else:
                    doshrink = True
            if doshrink:
                for j in range(1, self.N + 1):
                    sim[j] = sim[0] + 0.5 * (sim[j] - sim[0])
                self.state = "shrink"
                return
        else:
            raise RuntimeError("tell() on a finished run")
        self.iterations += 1
        self._sort()
        self._next()


def minimize_many(func_many, guesses, xtol=1e-4, ftol=1e-4, maxiter=None):
    """Independent downhill-simplex runs in lockstep: func_many([m, N] points) -> [m] values is called once per round with what
    every live run asks for.  Returns a list of (xopt, fopt, iterations), what scipy.optimize.fmin returns for each guess."""
    runs = [NelderMead(g, xtol=xtol, ftol=ftol, maxiter=maxiter) for g in guesses]
    while True:
        asks = [(r, r.ask()) for r in runs if not r.done]
        if not asks:
            break
        vals = np.asarray(func_many(np.concatenate([a for _, a in asks], axis=0)), dtype=float)
        at = 0
        for r, a in asks:
            r.tell(vals[at:at + len(a)])
            at += len(a)
    return [(r.x.copy(), float(r.fun), r.iterations) for r in runs]


# --------------------------------------------------------------------------- the calibration
class ReplayedVehicle:
    """What simulate_single(return_vehicles=True) hands back per sample: `traj` [6, n + 1] (column 0: the start state, column
    i: the state after tick i; rows the vehicle class lacks stay 0), `i` = n ticks, `s` the last state."""

    def __init__(self, traj, vid):
        self.traj = traj
        self.i = traj.shape[1] - 1
        self.s = traj[:, -1].copy()
        self.id = vid


class _Calibration:
    """What DownhillSimplexCalibration and InteractionCalibration share: the data sets loaded on first use and closed together, the
    chunk loop of `evaluate`, and `run_many`.  A class says how a data set is loaded (`_load` -> a mapping with "engine", "sets" and
    "objectives"), what a parameter vector becomes (`_candidates`), how a chunk of candidates is launched (`_launch`), how the
    device's sums become errors (`_errors`) and its states trajectories (`_trajs`)."""

    xtol = ftol = 1e-4                                            # (minimize_many's own defaults)

    def close(self):
        for ds in self._sets.values():
            ds["engine"].close()
        self._sets = {}

    def _dataset(self, test=False):
        """the engine that holds the training (test) data, loaded on first use"""
        ds = self._sets.get(bool(test))
        if ds is None:
            ds = self._sets[bool(test)] = self._load(self.test_data if test else self.train_data)
        return ds

    def evaluate(self, params_vals, test=False):
        """Errors of many parameter vectors, [k, n_params] -> [k]: one launch per max_sets of them.  With calc_sse_timesteps or
        calc_maesse_samples the error is formed from the sums the device returns; another error_func gets the trajectories."""
        vals = np.atleast_2d(np.asarray(params_vals, dtype=float))
        ds = self._dataset(test)
        cands = self._candidates(vals)
        err = np.zeros(len(cands))
        for at in range(0, len(cands), ds["sets"]):
            chunk = cands[at:at + ds["sets"]]
            if self.error_func is calc_sse_timesteps or self.error_func is calc_maesse_samples:
                err[at:at + len(chunk)] = self._errors(ds, self._launch(ds, chunk))
            else:
                _, states = self._launch(ds, chunk, states=True)
                for k in range(len(chunk)):
                    err[at + k] = self.error_func(self._trajs(ds, states, k), ds["objectives"])
        return err

    def run_many(self, guesses):
        """Independent calibrations from several guesses, in lockstep (minimize_many): every iteration of all live runs is one launch
        (a shrink one more).  Returns a list of (xopt, fopt, iterations) - per guess what `run` finds from it - and keeps the best in
        param_args_opt."""
        res = minimize_many(self.evaluate, [np.asarray(g, dtype=float) for g in guesses], xtol=self.xtol, ftol=self.ftol, maxiter=self.maxiter)
        best = min(res, key=lambda r: r[1])
        self.param_args_opt = self._update_params_args_dict(best[0])
        return res


class DownhillSimplexCalibration(_Calibration):
    """Fit parameters of a vehicle class to recorded trajectories by downhill simplex (calibration.py:243-526).  Arguments as the
    reference's; `device` and `max_sets` (parameter sets per launch, at most 256) are this package's."""

    def __init__(self, vehicle_type, params_keys, train_data, test_data, objective_features_traj, error_func=calc_sse_timesteps,
                 fix_speed=True, maxiter=100, params_auxfuncs=None, params_auxfuncsargs=None, verbose=True, device=0, max_sets=256):
        n_keys = len(params_keys)
        if params_auxfuncs is None:
            if params_auxfuncsargs is not None:
                raise ValueError("params_auxfuncsargs without params_auxfuncs")
        else:
            params_auxfuncs = list(params_auxfuncs)
            params_auxfuncsargs = [{} for _ in params_auxfuncs] if params_auxfuncsargs is None else list(params_auxfuncsargs)
            for name, lst in (("params_auxfuncs", params_auxfuncs), ("params_auxfuncsargs", params_auxfuncsargs)):
                if len(lst) != n_keys:
                    raise ValueError(f"{name} has {len(lst)} entries, params_keys names {n_keys} parameters")
        self.vehicle_type, self.params_keys = vehicle_type, params_keys
        self.params_auxfuncs, self.params_auxfuncsargs = params_auxfuncs, params_auxfuncsargs
        self.train_data, self.test_data = train_data, test_data
        self.objective_features_traj = _indicators(objective_features_traj, "objective_features_traj", TRAJ_ROWS)
        self.error_func, self.fix_speed, self.maxiter, self.verbose = error_func, fix_speed, maxiter, verbose
        self.param_args_opt = None
        self.device, self.max_sets = device, int(max_sets)
        self._sets = {}

    def _update_params_args_dict(self, params_vals):
        """the optimiser's vector -> keyword arguments of the vehicle class's parameter object: value k belongs to params_keys[k],
        or, with auxiliary functions, key k gets params_auxfuncs[k](params_vals, **params_auxfuncsargs[k])"""
        if self.params_auxfuncs is None:
            return dict(zip(self.params_keys, params_vals))
        return {key: fn(params_vals, **kw) for key, fn, kw in zip(self.params_keys, self.params_auxfuncs, self.params_auxfuncsargs)}

    def _pod(self, params_args):
        return self.vehicle_type.PARAMS_TYPE(**params_args).to_pod(self.vehicle_type.MODEL)

    def _load(self, data):
        samples = [(s0, np.asarray(i, dtype=float), np.asarray(o, dtype=float)) for s0, i, o in data]
        feat = np.flatnonzero(self.objective_features_traj).astype(np.int32)
        n_seq = len(samples)
        lens = np.array([i.shape[0] for _, i, _ in samples], dtype=np.int32)
        T = int(lens.max())
        Fx, Fy, obj = np.zeros((T, n_seq)), np.zeros((T, n_seq)), np.zeros((T, n_seq, feat.size))
        s0s = np.zeros((n_seq, 8))
        for k, (s0, inp, o) in enumerate(samples):
            if o.shape != (lens[k], feat.size):
                raise ValueError(f"sample {k}: the objective has shape {o.shape}, objective_features_traj selects {feat.size} rows of vehicle.traj")
            Fx[: lens[k], k], Fy[: lens[k], k], obj[: lens[k], k] = inp[:, 0], inp[:, 1], o
            s0s[k, :TRAJ_ROWS] = s0
        sets = max(1, min(self.max_sets, 256))
        engine = Engine(self._pod({}), sets * n_seq, device=self.device)
        engine.calib_load(s0s, Fx, Fy, obj, feat, lengths=lens, max_sets=sets)
        return dict(engine=engine, lens=lens, feat=feat, n_seq=n_seq, sets=sets, s0=s0s, objectives=[o for _, _, o in samples])

    def _candidates(self, vals):
        return [self._pod(self._update_params_args_dict(v)) for v in vals]

    def _launch(self, ds, pods, **kw):
        return ds["engine"].calib_eval(pods, fix_speed=self.fix_speed, **kw)

    def _errors(self, ds, sums):
        if self.error_func is calc_sse_timesteps:
            return sums[:, :, 0].sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):       # (an empty sample: nan, as np.mean gives)
            return ((sums[:, :, 1] / (ds["lens"] * float(ds["feat"].size))[None, :]) ** 2).sum(axis=1)

    def _trajs(self, ds, states, k):
        """the samples of parameter set k from the states of one evaluation: [len, n_feat] each (rows the class lacks: 0)"""
        ns = states.shape[2]
        out = []
        for q in range(ds["n_seq"]):
            tr = np.zeros((ds["lens"][q], ds["feat"].size))
            for c, f in enumerate(ds["feat"]):
                if f < ns:
                    tr[:, c] = states[: ds["lens"][q], k * ds["n_seq"] + q, f]
            out.append(tr)
        return out

    def simulate_single(self, params_args, return_vehicles=False, test=False):
        """One parameter set on every sample of the training (test) data (calibration.py:397-470): the samples' trajectories
        [n, n_feat] - the state after each tick - or, with return_vehicles, ReplayedVehicle objects; and the objectives."""
        ds = self._dataset(test)
        _, states = ds["engine"].calib_eval([self._pod(params_args)], fix_speed=self.fix_speed, states=True)
        if not return_vehicles:
            return self._trajs(ds, states, 0), list(ds["objectives"])
        ns = states.shape[2]
        vehicles = []
        for q in range(ds["n_seq"]):
            n = int(ds["lens"][q])
            traj = np.zeros((TRAJ_ROWS, n + 1))
            traj[:, 0] = ds["s0"][q, :TRAJ_ROWS]
            traj[: min(ns, TRAJ_ROWS), 1:] = states[:n, q, :TRAJ_ROWS].T
            vehicles.append(ReplayedVehicle(traj, self.vehicle_type.__name__))
        return vehicles, list(ds["objectives"])

    def run(self, params_vals_guess):
        """The calibration by scipy.optimize.fmin, as the reference runs it (calibration.py:472-526): returns fmin's full output
        with the samples replayed at the optimum appended."""
        from scipy.optimize import fmin

        if self.verbose:
            print(f"Calibrating {self.vehicle_type.__name__} ...")
        results = list(fmin(objective_function_wrapper, params_vals_guess, (self,), full_output=True, maxiter=self.maxiter,
                            disp=bool(self.verbose)))
        param_args = self._update_params_args_dict(results[0])
        if self.verbose:
            for key in param_args.keys():
                print(f"         {key}: {param_args[key]}")
        results.append(self.simulate_single(param_args, return_vehicles=True))
        self.param_args_opt = param_args
        return results

    def test(self, param_args_opt=None, plot_results=False, color="blue", axes=None, name=None, plot_inref=True):
        """Error of a parameter set - by default the one `run` / `run_many` found - on the TEST data; returns (error, vehicles).
        The plotting arguments of the reference's signature are accepted; plotting itself is not part of this package."""
        if plot_results:
            raise NotImplementedError("DownhillSimplexCalibration.test: plotting is not provided; plot the returned vehicles' traj")
        args = self.param_args_opt if param_args_opt is None else param_args_opt
        if args is None:
            raise RuntimeError("no parameters to test: call run() or run_many() first, or pass param_args_opt")
        vehicles, objectives = self.simulate_single(args, test=True, return_vehicles=True)
        rows = self.objective_features_traj
        error = self.error_func([v.traj[rows, 1: v.i + 1].T for v in vehicles], objectives)
        if self.verbose:
            print(f"test error on {len(vehicles)} samples: {error:.6g}")
        return error, vehicles


# --------------------------------------------------------------------------- interaction parameters, closed loop
class SceneData:
    """One recorded scene of road users that interact - up to 32 of them, or any number on its roster with presence windows that keep
    at most 32 in the scene at any tick - (plain arrays): start states s0 [n, >= 4] (x, y, psi, v, ...),
    desired speeds v_desired [n] (or a scalar), the riders' destination queues in CSR form (dest_offsets [n + 1], dest_xyz_stop
    [rows, 3] = (x, y, stop); at least one row each), the recorded trajectory traj [n_t, n, n_cols] - row t the state AFTER tick
    t + 1, columns the rows of vehicle.traj (x, y, psi, v, delta, theta) as far as they were recorded - and its length in ticks
    (default: n_t).

    replayed [n] (bool, default: nobody) marks road users that FOLLOW THEIR RECORDING: they are not simulated with the candidate
    parameters but put on traj[t, i, :4] = (x, y, psi, v) after every tick, act on the others as sources of the field only and
    add nothing to the error - the others of an ego evaluation (`ego_split`), or a road user of another class.  Such a road
    user needs finite columns 0 .. 3 of traj over all `length` rows; its destination queue may be left out (no row between its
    two offsets): it gets the single row a fresh vehicle has, its own start (vehicle.py:183-185).

    road = (offsets [n_edges + 1], verts [n_v, 2], F0 [n_edges], sigma [n_edges]) gives the scene ROAD EDGES, as `Engine.set_road`
    takes them (default: none): every tick adds their force to every simulated road user (intersection.py:226-242, 853-857).  All
    edges together have at most ROAD_MAX_VERTS vertices and, padded to a multiple of 64, at most 16 384 / P of them, P the power of two
    that holds the scene's road users - what the one-wave tick stages.

    present = (enter [n], exit [n]) gives every road user a PRESENCE WINDOW [enter, exit) in ticks of the scene, 0 <= enter <= exit
    <= length (default: all of [0, length)).  At a tick outside its window a road user is not in the scene: it is neither a source
    nor a receiver of the field, it is not ticked or put on its recording, and nothing is added to its error.  s0 of a road user is
    its state at the start of tick `enter` (a fresh vehicle joins there: intersection.add_vehicle between two steps); after `exit`
    it keeps its last state.  enter == exit: never present.  traj outside a road user's window is never read and may be NaN; a
    replayed road user needs finite (x, y, psi, v) inside its window only.

    A roster above 32 needs `present`, and at no tick more than 32 road users whose window holds it (ValueError names the tick and the
    count; a road user with an empty window counts for nothing).  Such a scene runs on `lanes()`: road users whose windows do not
    overlap take turns on one lane of the one-wave tick.  Its road limit is that of the power of two that holds its LANES.

    wide=True lifts the bound to 256 road users AT ONCE (`Engine.scene_calib_load_wide`: one workgroup of 256 threads ticks such a scene).
    A roster above 32 then needs no `present` - without windows `lanes()` gives lane = index -, the ValueError names tick and count
    against 256, and the road limit is that of P = 64, 128 or 256, the power of two that holds its lanes and at least 64: 256, 128 or
    64 vertices (padded to a multiple of 64), whichever kernel the scene ends up on.  With the default wide=False nothing changes.

    group [n] (integers >= 0, default: everybody 0) puts every road user into a GROUP that carries parameters of its own - e-bikes and
    city bikes, commuters and children (`InteractionCalibration(group_params=...)`, `Engine.scene_calib_groups`): a road user is
    simulated with its group's parameter set and acts on the others with that set's field and field of view, replayed or not."""

    ROAD_MAX_VERTS = 2048

    WIDE_MAX = 256

    def __init__(self, s0, v_desired, dest_offsets, dest_xyz_stop, traj, length=None, replayed=None, road=None, present=None, wide=False,
                 group=None):
        # one step per layer, in the order that decides which message an input with two faults gets
        self.wide = bool(wide)
        self._take_roster(s0, present is not None)
        self._take_v_desired(v_desired)
        self._take_group(group)
        self._take_replayed(replayed)
        self._take_queues(dest_offsets, dest_xyz_stop)
        self._take_traj(traj, length)
        self._take_windows(present)
        self._check_peak()
        self._check_replay()
        self.road = None if road is None else self._checked_road(road, self.n if self.n <= 32 else self.lanes()[1],
                                                                 p_min=64 if self.wide else 1)   # (a workgroup's P: never below a wave)

    def _take_roster(self, s0, windows):
        self.s0 = np.asarray(s0, dtype=float)
        self._most = most = self.WIDE_MAX if self.wide else 32    # road users in the scene at once
        if self.s0.ndim != 2 or self.s0.shape[1] < 4 or self.s0.shape[0] < 1 or (self.s0.shape[0] > most and not windows):
            raise ValueError(f"a {'wide ' if self.wide else ''}scene has 1 .. {most} road users, or more with presence windows that keep at most "
                             f"{most} at once: s0 is [n, >= 4]")

    def _take_v_desired(self, v_desired):
        try:
            self.v_desired = np.array(np.broadcast_to(np.asarray(v_desired, dtype=float), (self.n,)))
        except ValueError:
            raise ValueError("v_desired: one desired speed per road user, or a scalar") from None

    def _take_group(self, group):
        self.grouped = group is not None
        g = np.zeros(self.n, dtype=np.int32) if group is None else np.asarray(group)
        if g.shape != (self.n,) or g.dtype.kind not in "iu":
            raise ValueError("group: one integer per road user")
        if np.any(g < 0):
            raise ValueError("group: entries are >= 0")
        self.group = g.astype(np.int32)

    def _take_replayed(self, replayed):
        self.replayed = np.zeros(self.n, dtype=bool) if replayed is None else np.array(replayed, dtype=bool)
        if self.replayed.shape != (self.n,):
            raise ValueError("replayed: one flag per road user")

    def _take_queues(self, dest_offsets, dest_xyz_stop):
        n = self.n
        self.dest_offsets = np.asarray(dest_offsets, dtype=np.int64)
        self.dest_xyz_stop = np.asarray(dest_xyz_stop, dtype=float).reshape(-1, 3)
        off = self.dest_offsets
        if off.shape != (n + 1,) or off[0] != 0 or off[-1] != self.dest_xyz_stop.shape[0] or np.any(np.diff(off) < 0) \
                or np.any((np.diff(off) < 1) & ~self.replayed):
            raise ValueError("dest_offsets is [n + 1], starts at 0, ends at the rows of dest_xyz_stop, and gives every simulated road user a row")
        if np.any(np.diff(off) < 1):                              # a replayed road user without a queue: its own start, no stop
            rows, new = [], [0]
            for i in range(n):
                own = self.dest_xyz_stop[off[i]: off[i + 1]]
                rows.append(own if own.shape[0] else np.array([[self.s0[i, 0], self.s0[i, 1], 0.0]]))
                new.append(new[-1] + rows[-1].shape[0])
            self.dest_offsets, self.dest_xyz_stop = np.array(new, dtype=np.int64), np.concatenate(rows)

    def _take_traj(self, traj, length):
        self.traj = np.asarray(traj, dtype=float)
        if self.traj.ndim != 3 or self.traj.shape[1] != self.n or not 1 <= self.traj.shape[2] <= TRAJ_ROWS:
            raise ValueError(f"traj is [n_t, n, 1 .. {TRAJ_ROWS}]: the state of every road user after every tick")
        self.length = self.traj.shape[0] if length is None else int(length)
        if not 0 <= self.length <= self.traj.shape[0]:
            raise ValueError("length: 0 .. the rows of traj")

    def _take_windows(self, present):
        n = self.n
        try:                                                      # (default: everybody over all of [0, length))
            enter, exit_ = (np.zeros(n, dtype=np.int32), np.full(n, self.length, dtype=np.int32)) if present is None else present
            enter, exit_ = np.asarray(enter), np.asarray(exit_)
        except (TypeError, ValueError):
            raise ValueError("present is (enter [n], exit [n])") from None
        if enter.shape != (n,) or exit_.shape != (n,) or enter.dtype.kind not in "iu" or exit_.dtype.kind not in "iu":
            raise ValueError("present: one integer entry tick and one integer exit tick per road user")
        if np.any(enter < 0) or np.any(enter > exit_) or np.any(exit_ > self.length):
            raise ValueError("present: 0 <= enter <= exit <= length for every road user")
        self.enter, self.exit = enter.astype(np.int32), exit_.astype(np.int32)
        self.windowed = bool(np.any(self.enter != 0) or np.any(self.exit != self.length))

    def _check_peak(self):
        """a roster above the bound: at no tick more road users in the scene than the bound"""
        if self.n > self._most:
            count = self.inside.sum(axis=1) if self.length else np.zeros(1, dtype=int)
            if count.max() > self._most:
                raise ValueError(f"present: {int(count.max())} road users are in the scene at tick {int(count.argmax())}; at most {self._most} at once")

    def _check_replay(self):
        """a replayed road user has finite (x, y, psi, v) wherever it is put on its recording"""
        if not self.replayed.any():
            return
        if self.traj.shape[2] < 4:
            raise ValueError("a replayed road user needs (x, y, psi, v): traj has fewer than 4 columns")
        if not self.windowed:
            finite = np.isfinite(self.traj[: self.length][:, self.replayed, :4]).all()
        else:
            finite = all(np.isfinite(self.traj[self.enter[i]: self.exit[i], i, :4]).all() for i in np.flatnonzero(self.replayed))
        if not finite:
            raise ValueError("a replayed road user needs finite (x, y, psi, v) - columns 0 .. 3 of traj - over the rows of its window "
                             "(all `length` rows without one)")

    @classmethod
    def _checked_road(cls, road, n, p_min=1):
        try:
            roff, verts, F0, sigma = road
        except (TypeError, ValueError):
            raise ValueError("road is (offsets, verts, F0, sigma)") from None
        roff = np.array(roff, dtype=np.int64).reshape(-1)
        verts = np.array(verts, dtype=float).reshape(-1, 2)
        n_edges = roff.size - 1
        if n_edges < 0 or np.any(roff < 0) or np.any(np.diff(roff) < 0) or (roff.size and roff[-1] > verts.shape[0]):
            raise ValueError("road: offsets is [n_edges + 1], ascending, within the vertices")
        try:
            F0 = np.array(np.broadcast_to(np.asarray(F0, dtype=float), (n_edges,)))
            sigma = np.array(np.broadcast_to(np.asarray(sigma, dtype=float), (n_edges,)))
        except ValueError:
            raise ValueError("road: one F0 and one sigma per edge, or scalars") from None
        used = np.concatenate([verts[roff[k]: roff[k + 1]] for k in range(n_edges)]) if n_edges else verts[:0]
        if not (np.isfinite(used).all() and np.isfinite(F0).all() and np.isfinite(sigma).all()):
            raise ValueError("road: vertices, F0 and sigma must be finite")
        nv = used.shape[0]
        P = p_min
        while P < n:
            P *= 2
        if nv > cls.ROAD_MAX_VERTS or (nv + 63) // 64 * 64 * P > 256 * 64:
            raise ValueError(f"road: {nv} vertices; a scene of {n} road users takes {min(cls.ROAD_MAX_VERTS, 256 * 64 // P)}")
        return roff, verts, F0, sigma

    @property
    def n(self):
        return self.s0.shape[0]

    @property
    def inside(self):
        """[length, n] bool: road user i is present at tick t"""
        t = np.arange(self.length)[:, None]
        return (self.enter[None, :] <= t) & (t < self.exit[None, :])

    def lanes(self):
        """(lane [n] int32, n_lanes): road users whose windows do not overlap share a lane.  In order of (enter, roster index) every
        road user takes the lowest lane whose last occupant has exit <= enter - for intervals that is optimal, so n_lanes is the
        largest number present at once (at least 1).  A road user with an empty window occupies nothing: lane 0."""
        lane, last = np.zeros(self.n, dtype=np.int32), []
        for i in sorted(np.flatnonzero(self.exit > self.enter).tolist(), key=lambda i: (int(self.enter[i]), i)):
            for k, x in enumerate(last):
                if x <= self.enter[i]:
                    break
            else:
                k = len(last)
                last.append(0)
            lane[i], last[k] = k, int(self.exit[i])
        return lane, max(1, len(last))

    def replay_rows(self):
        """[n_t, replayed road users, 4]: the recorded (x, y, psi, v) as `Engine.scene_calib_replay` takes them.  Without windows
        that is traj itself.  Outside its window a row is never used, but the engine wants the rows of a scene finite: there a road
        user gets the nearest row inside its window (one that is never present: its start state)."""
        rows = self.traj[:, self.replayed, :4]
        if self.windowed:
            rows = rows.copy()
            for c, i in enumerate(np.flatnonzero(self.replayed)):
                a, b = int(self.enter[i]), int(self.exit[i])
                rows[:a, c] = self.traj[a, i, :4] if a < b else self.s0[i, :4]
                rows[b: self.length, c] = self.traj[b - 1, i, :4] if a < b else self.s0[i, :4]
        return rows

    def ego_split(self):
        """The leave-one-out scenes of this scene, one per simulated road user: scene i simulates that road user alone and replays
        all others from the recording (road users that are replayed here stay so).  Host only.  s0, the queues and traj are
        shared with this scene, not copied; every scene has a mask of its own and this scene's road and presence windows."""
        out = []
        wide = dict(wide=True) if self.wide else {}
        if self.grouped:
            wide["group"] = self.group
        # (a road user that is never present in a scene that has ticks is nobody's ego)
        for i in np.flatnonzero(~self.replayed & ((self.exit > self.enter) | (self.length == 0))):
            mask = np.ones(self.n, dtype=bool)
            mask[i] = False
            out.append(SceneData(self.s0, self.v_desired, self.dest_offsets, self.dest_xyz_stop, self.traj, length=self.length, replayed=mask,
                                 road=self.road, present=(self.enter, self.exit) if self.windowed or self.n > 32 else None, **wide))
        return out


def _init_names(cls):
    """the keyword arguments the constructor of a PARAMS_TYPE takes, its base classes' included where it passes **kwargs on"""
    import inspect
    names = set()
    for c in cls.__mro__:
        if "__init__" not in vars(c):
            continue
        sig = inspect.signature(c.__init__).parameters
        names |= {n for n, q in sig.items() if n != "self" and q.kind in (q.POSITIONAL_OR_KEYWORD, q.KEYWORD_ONLY)}
        if not any(q.kind == q.VAR_KEYWORD for q in sig.values()):
            break
    return names


def _has_road(data):
    """a scene of the data set has a road with at least one vertex"""
    return any(d.road is not None and d.road[0][-1] > 0 for d in data)


def _riders_then_scenes(per_rider, roff):
    """[k, R] per-rider figures -> [k, n_scn]: the riders of a scene added in rider order (the order of the sum is fixed)"""
    out = np.zeros((per_rider.shape[0], len(roff) - 1))
    for q in range(len(roff) - 1):
        for r in range(roff[q], roff[q + 1]):
            out[:, q] += per_rider[:, r]
    return out


def _scenes_in_order(per_scene):
    acc = np.zeros(per_scene.shape[0])
    for q in range(per_scene.shape[1]):
        acc += per_scene[:, q]
    return acc


class InteractionCalibration(_Calibration):
    """Fit parameters that act BETWEEN road users - the social-force field f_0, sigma_0..3, e_0, e_1, hfov, p_0, p_decay, the priority
    rule - to recorded scenes by downhill simplex.  A replay of recorded forces (DownhillSimplexCalibration) couples no two vehicles;
    here every candidate set simulates every scene with its road users together, on the device: the scenes are loaded once
    (`Engine.scene_calib_load`) and an evaluation of the objective is one launch for all scenes and up to `max_sets` (at most 256)
    candidate sets (`Engine.scene_calib_eval`).  With calc_sse_timesteps or calc_maesse_samples the error is formed from the
    per-rider sums the device returns - the riders of a scene added in rider order, then the scenes in scene order; a sample of
    calc_maesse_samples is a scene - and another error_func gets the trajectories, [length, n_riders, n_feat] per scene.

    Road users a scene marks as replayed (`SceneData(replayed=...)`, `SceneData.ego_split`) follow their recording on the device
    (`Engine.scene_calib_replay`) and are no part of the error: calc_sse_timesteps sums the simulated riders, calc_maesse_samples
    divides a scene's sum by length x simulated riders x n_feat, another error_func and `simulate` get the simulated riders only.

    Scenes with road edges (`SceneData(road=...)`) are loaded with their roads (`Engine.scene_calib_road`).  "road_F_0" and
    "road_sigma" among params_keys fit the two RoadElementParameters of the road-edge force: they go to the evaluation's road
    overrides, one value per candidate set for every edge of every scene, and not into PARAMS_TYPE; with only one of them fitted the
    other keeps its value from RoadElementParameters().  Either key needs a scene with a road (ValueError otherwise).

    Scenes whose road users enter and leave (`SceneData(present=...)`) are loaded with their windows (`Engine.scene_calib_windows`) and
    the launch honours them.  Both built-in errors are formed over the present (rider, tick) cells: calc_sse_timesteps sums them,
    calc_maesse_samples divides a scene's sum by n_feat x the present cells of its simulated riders.  Another error_func and
    `simulate` get NaN outside a rider's window, in the trajectories and in the objectives alike.

    A scene whose roster exceeds 32 runs on shared lanes (`SceneData.lanes`, `Engine.scene_calib_load_shared`): the whole data set is
    then loaded with one such call, every scene on its lanes, and the windows go with the load.  share_lanes=True asks for that
    whatever the rosters - fewer lanes than road users make the pair loops narrower.  Errors, `simulate` and a custom error_func are
    what they are with windows: present cells only, NaN outside.

    A data set with a scene marked `SceneData(wide=True)` - up to 256 road users at once - is loaded by `Engine.scene_calib_load_wide`:
    every scene on its lanes as above, the scenes with at least `wide_from` lanes on the workgroup kernel and the others on the one-wave
    tick; an evaluation is then up to two launches.  wide_from = 33 is the smallest scene the one-wave tick cannot take, not a measured
    crossover.  Errors, `simulate`, a custom error_func, NaN outside windows and the road keys are what they are under shared lanes.

    Road users in GROUPS with parameters of their own (`SceneData(group=...)`): group_params is a list of G dicts of FIXED keyword
    arguments of PARAMS_TYPE, one per group - what is known to differ between the groups; its length defines G (at most 4).  An entry
    of params_keys is then either "name" - fitted, one value shared by all groups - or ("name", g) - fitted for group g alone; the road
    keys stay per candidate.  A candidate vector becomes G parameter sets, PARAMS_TYPE(**group_params[g], **shared, **own[g]), and an
    evaluation is `Engine.scene_calib_eval_groups`.  Both built-in errors, `simulate`, `test` and a custom error_func are per road
    user and work as without groups.  Groups need `Engine.scene_calib_load`: with shared lanes or a wide scene a ValueError says so -
    unless lane_groups=True, which loads such a data set as above and then hands the groups to `Engine.scene_calib_lane_groups`: a lane
    then carries the parameters of the rider it holds.  Without group_params nothing changes and no new call is made.

    Road users of SEVERAL VEHICLE CLASSES, all simulated: vehicle_type is then a list or tuple of G vehicle types, group g
    of `SceneData(group=...)` being of class vehicle_type[g] - a Bicycle among TwoDBicycles, a BalancingRiderBicycle among
    InvPendulumBicycles.  group_params defaults to G empty dicts and must have length G, at most 12 (six classes x two kinds of rider);
    ("name", g) fits a parameter of group g's PARAMS_TYPE, "name" one value shared by all groups - it must be a parameter of EVERY
    group's PARAMS_TYPE (ValueError names key and group).  Record g of a candidate is vehicle_type[g].PARAMS_TYPE(...).to_pod(
    vehicle_type[g].MODEL); the data set is loaded by `Engine.scene_calib_load` and then `Engine.scene_calib_classes`, and everything
    else - both built-in errors, a custom error_func, `simulate`, `run`, `run_many`, `test`, replay, windows, roads and the road keys -
    works as with groups.  Mixed classes run on Engine.scene_calib_load only: a data set that needs shared lanes or a wide scene raises
    ValueError - unless lane_classes=True, which loads such a data set on its lanes as above and then hands groups,
    classes and start states to `Engine.scene_calib_lane_classes`: a lane then carries the class of the rider it holds and changes it
    at a takeover.  With a single vehicle_type, or on a plain load, nothing changes and no new call is made.

    train_data, test_data: lists of SceneData; objective_features_traj: six indicators over the rows of vehicle.traj."""

    ROAD_KEYS = {"road_F_0": "F_0", "road_sigma": "sigma"}

    def __init__(self, vehicle_type, params_keys, train_data, test_data, objective_features_traj, error_func=calc_sse_timesteps,
                 max_sets=256, maxiter=100, xtol=1e-4, ftol=1e-4, verbose=False, device=0, engine_factory=Engine, share_lanes=False,
                 wide_from=33, group_params=None, lane_groups=False, lane_classes=False):
        self.vehicle_type, self.params_keys = vehicle_type, list(params_keys)
        self._take_groups(vehicle_type, group_params)
        self._check_keys()
        self.share_lanes, self.lane_groups, self.wide_from = bool(share_lanes), bool(lane_groups), int(wide_from)
        self.lane_classes = bool(lane_classes)
        if not 1 <= self.wide_from <= SceneData.WIDE_MAX + 1:
            raise ValueError(f"wide_from: 1 .. {SceneData.WIDE_MAX + 1}")
        self.train_data, self.test_data = list(train_data), list(test_data)
        self._check_data()
        self.objective_features_traj = _indicators(objective_features_traj, "objective_features_traj", TRAJ_ROWS)
        if not self.objective_features_traj.any():
            raise ValueError("objective_features_traj selects no row of vehicle.traj")
        self.error_func, self.maxiter, self.xtol, self.ftol, self.verbose = error_func, maxiter, xtol, ftol, verbose
        self.device, self.max_sets = device, max(1, min(int(max_sets), 256))
        self.param_args_opt = None
        self._factory = engine_factory
        self._sets = {}
        self._road_keys = [k for k in self.params_keys if k in self.ROAD_KEYS]
        if self._road_keys:                                       # either road key needs a scene with a road
            for name, data in (("train_data", self.train_data), ("test_data", self.test_data)):
                if data and not _has_road(data):
                    raise ValueError(f"params_keys names {self._road_keys}, and no scene of {name} has a road")

    def _take_groups(self, vehicle_type, group_params):
        """the vehicle classes (`_types`; None: one class), the groups' fixed arguments and their number `_G`"""
        self._types = list(vehicle_type) if isinstance(vehicle_type, (list, tuple)) else None      # several vehicle classes: one per group
        if self._types is not None:
            if not 2 <= len(self._types) <= 12:
                raise ValueError("vehicle_type: a vehicle type, or a list of 2 .. 12 of them - one per group")
            for g, t in enumerate(self._types):
                if getattr(t, "MODEL", None) is None or t.MODEL == _ffi.UNCONTROLLED:
                    raise ValueError(f"vehicle_type[{g}]: {getattr(t, '__name__', t)!r} is not one of the six simulated vehicle classes")
            if group_params is None:
                group_params = [{} for _ in self._types]
            if len(group_params) != len(self._types):
                raise ValueError(f"group_params: {len(group_params)} dicts for {len(self._types)} vehicle types - one per group")
        self.group_params = None if group_params is None else [dict(g) for g in group_params]
        self._G = 1 if self.group_params is None else len(self.group_params)
        if self._types is None and not 1 <= self._G <= 4:
            raise ValueError("group_params: 1 .. 4 dicts of keyword arguments of PARAMS_TYPE, one per group")

    def _check_keys(self):
        """the grammar of params_keys - "name" or ("name", group) - and, with several vehicle classes, that a key is a parameter of the
        PARAMS_TYPE of every group it reaches.  A fault of the grammar in ANY key is named before a key that is no parameter: the
        parameters are looked up once the grammar has been through."""
        for k in self.params_keys:
            if isinstance(k, str):
                continue
            if not (isinstance(k, tuple) and len(k) == 2 and isinstance(k[0], str) and isinstance(k[1], (int, np.integer))
                    and not isinstance(k[1], bool)):
                raise ValueError(f"params_keys: {k!r} is neither \"name\" nor (\"name\", group)")
            if k[0] in self.ROAD_KEYS:
                raise ValueError(f"params_keys: {k!r}: the road keys are per candidate set, not per group")
            if self.group_params is None:
                raise ValueError(f"params_keys: {k!r} names a group and there is no group_params")
            if not 0 <= k[1] < self._G:
                raise ValueError(f"params_keys: {k!r} names group {k[1]}, group_params defines {self._G}")
        if self._types is None:
            return
        for k in self.params_keys:
            name = k if isinstance(k, str) else k[0]
            if name in self.ROAD_KEYS:
                continue
            for g in (range(self._G) if isinstance(k, str) else (k[1],)):
                if name not in _init_names(self._types[g].PARAMS_TYPE):
                    raise ValueError(f"params_keys: {k!r}: {name!r} is no parameter of {self._types[g].PARAMS_TYPE.__name__}, "
                                     f"the PARAMS_TYPE of group {g} ({self._types[g].__name__})")

    def _check_data(self):
        for d in self.train_data + self.test_data:
            if not isinstance(d, SceneData):
                raise TypeError("train_data and test_data are lists of SceneData")
        for name, data in (("train_data", self.train_data), ("test_data", self.test_data)):
            for q, d in enumerate(data):
                if d.group.max() >= self._G:
                    raise ValueError(f"scene {q} of {name} has a road user in group {int(d.group.max())}, group_params defines {self._G} "
                                     f"group{'s' if self._G > 1 else ''}")
        if not self.train_data:
            raise ValueError("no scenes to train on")

    def _update_params_args_dict(self, params_vals):
        return dict(zip(self.params_keys, params_vals))

    def _pod(self, params_args):
        return self.vehicle_type.PARAMS_TYPE(**{k: v for k, v in params_args.items() if k not in self.ROAD_KEYS}).to_pod(self.vehicle_type.MODEL)

    def _group_args(self, params_args):
        """the keyword arguments of PARAMS_TYPE per group: group_params[g], the shared keys, the group's own"""
        shared = {k: v for k, v in params_args.items() if isinstance(k, str) and k not in self.ROAD_KEYS}
        return [{**self.group_params[g], **shared, **{k[0]: v for k, v in params_args.items() if isinstance(k, tuple) and k[1] == g}}
                for g in range(self._G)]

    def _pods(self, params_args):
        """a candidate as Engine.scene_calib_eval_groups takes it: one parameter set per group"""
        if self._types is not None:                               # (several vehicle classes: record g is of vehicle_type[g]'s)
            out = []
            for g, (t, a) in enumerate(zip(self._types, self._group_args(params_args))):
                try:
                    out.append(t.PARAMS_TYPE(**a).to_pod(t.MODEL))
                except TypeError as exc:
                    bad = [k for k in a if k not in _init_names(t.PARAMS_TYPE)]
                    raise ValueError(f"group {g} ({t.__name__}): {bad or sorted(a)} - {exc}") from None
            return tuple(out)
        return tuple(self.vehicle_type.PARAMS_TYPE(**a).to_pod(self.vehicle_type.MODEL) for a in self._group_args(params_args))

    def _eval(self, ds, args_list, **kw):
        """one evaluation of the candidates args_list: Engine.scene_calib_eval, or - with groups - scene_calib_eval_groups"""
        if self._G > 1:
            return ds["engine"].scene_calib_eval_groups([self._pods(a) for a in args_list], **kw)
        return ds["engine"].scene_calib_eval([self._pod(a) for a in args_list], **kw)

    def _road_over(self, args_list):
        """road_F0, road_sigma [n_sets] of an evaluation (keyword arguments of Engine.scene_calib_eval); {}: no road key is fitted"""
        if not self._road_keys:
            return {}
        rp = [RoadElementParameters(**{self.ROAD_KEYS[k]: float(a[k]) for k in self._road_keys}) for a in args_list]
        return dict(road_F0=np.array([r.F_0 for r in rp], dtype=float), road_sigma=np.array([r.sigma for r in rp], dtype=float))

    # ---- loading a data set: one step per layer of the host library (SceneImage, SceneLanes, SceneGroups, SceneReplay,
    # SceneRoad, SceneWindows), in the order the engine is called, and the host's own bookkeeping last
    def _load(self, data):
        if not data:
            raise ValueError("no test scenes")
        img = self._image(data, np.flatnonzero(self.objective_features_traj).astype(np.int32))
        engine, shared = self._load_image(data, img)
        self._load_replay(engine, data, img)
        self._load_road(engine, data)
        inside = self._load_windows(engine, data, img, shared)
        return self._bookkeeping(engine, data, img, inside)

    def _image(self, data, feat):
        """IMAGE: the scenes refused one by one, in scene order, and their arrays concatenated in rider order - each once"""
        nr = np.array([d.n for d in data], dtype=np.int32)
        roff = np.r_[0, np.cumsum(nr)].astype(np.int64)
        R, T = int(roff[-1]), max(1, max(d.traj.shape[0] for d in data))
        s0, vd, obj = np.zeros((R, 8)), np.zeros(R), np.zeros((T, R, feat.size))
        off, rows = [0], []
        for q, d in enumerate(data):
            if d.replayed.all():
                raise ValueError(f"scene {q}: every road user is replayed - there is nothing to fit")
            # (an empty scene - length 0 - stays what it was: no tick, no error; a scene that HAS ticks needs somebody to simulate)
            if d.length > 0 and not np.any(~d.replayed & (d.exit > d.enter)):
                raise ValueError(f"scene {q}: no simulated road user is ever present - there is nothing to fit")
            if feat.max() >= d.traj.shape[2]:
                raise ValueError(f"scene {q}: objective_features_traj names row {int(feat.max())} of vehicle.traj, the recorded trajectory has {d.traj.shape[2]}")
            sl = slice(roff[q], roff[q + 1])
            s0[sl, : min(d.s0.shape[1], 8)] = d.s0[:, :8]
            vd[sl] = d.v_desired
            obj[: d.traj.shape[0], sl] = d.traj[:, :, feat]
            off.extend((d.dest_offsets[1:] + len(rows)).tolist())
            rows.extend(d.dest_xyz_stop.tolist())
        per_rider = {name: np.concatenate([getattr(d, name) for d in data]) for name in ("enter", "exit", "group", "replayed")}
        return _Namespace(feat=feat, nr=nr, roff=roff, R=R, T=T, lens=np.array([d.length for d in data], dtype=np.int32), s0=s0, vd=vd,
                          off=np.array(off, dtype=np.int64), rows=np.array(rows, dtype=float).reshape(-1, 3), obj=obj, **per_rider)

    def _load_image(self, data, img):
        """LOAD: which of the three load calls the data set needs - refused before any engine is made where groups or classes cannot
        go with it -, the engine, that one load call and at most one call that hands over groups or classes; -> (engine, shared)"""
        wide = any(d.wide for d in data)
        shared = wide or self.share_lanes or any(d.n > 32 for d in data)
        needs = "this data set needs shared lanes" + (" and a wide scene" if wide else "") + " (a roster above 32, share_lanes or wide=True)"
        if self._types is not None and shared and not self.lane_classes:
            raise ValueError("mixed classes run on Engine.scene_calib_load only, and " + needs)
        if self._types is None and self._G > 1 and shared and not self.lane_groups:
            raise ValueError("group_params: rider groups run on Engine.scene_calib_load only, and " + needs + "; or pass lane_groups=True")
        pod0 = self._pods({})[0] if self._G > 1 else self._pod({})
        image = (img.s0, img.vd, img.off, img.rows, img.obj, img.feat)
        if shared:                                               # every scene on its lanes; the windows go with the load
            packed = [d.lanes() for d in data]
            nl = np.array([p[1] for p in packed], dtype=np.int32)
            engine = self._factory(pod0, max(img.R, self.max_sets * int(nl.sum())), device=self.device)
            load = engine.scene_calib_load_wide if wide else engine.scene_calib_load_shared
            load(img.nr, nl, np.concatenate([p[0] for p in packed]), img.enter, img.exit, *image, lengths=img.lens, max_sets=self.max_sets,
                 **(dict(wide_from=self.wide_from) if wide else {}))
            if self._types is not None:                          # (lane_classes=True: the class goes with the rider a lane carries)
                engine.scene_calib_lane_classes(img.group, [t.MODEL for t in self._types], img.s0)
            elif self._G > 1:                                    # (lane_groups=True: the group goes with the rider a lane carries)
                engine.scene_calib_lane_groups(img.group, self._G)
        else:
            engine = self._factory(pod0, self.max_sets * img.R, device=self.device)
            engine.scene_calib_load(img.nr, *image, lengths=img.lens, max_sets=self.max_sets)
            if self._types is not None:
                engine.scene_calib_classes(img.group, [t.MODEL for t in self._types], img.s0)
            elif self._G > 1:
                engine.scene_calib_groups(img.group, self._G)
        return engine, shared

    def _load_replay(self, engine, data, img):
        """REPLAY: the recorded (x, y, psi, v) of the replayed riders, in rider order - where anybody is replayed"""
        if not img.replayed.any():
            return
        rec = np.zeros((img.T, int(img.replayed.sum()), 4))
        at = 0
        for d in data:
            k = int(d.replayed.sum())
            if k:
                rec[: d.traj.shape[0], at: at + k] = d.replay_rows()
            at += k
        engine.scene_calib_replay(img.replayed, rec)

    def _load_road(self, engine, data):
        """ROAD: the edges of all scenes in one CSR, every edge with its scene - where a scene has a road"""
        if not _has_road(data):
            return
        edges = [(q, d.road[1][a:b], f0, sigma) for q, d in enumerate(data) if d.road is not None     # (scene, vertices, F0, sigma) per edge
                 for a, b, f0, sigma in zip(d.road[0][:-1], d.road[0][1:], d.road[2], d.road[3])]
        es, vs, f0, sg = zip(*edges)
        ro = np.r_[0, np.cumsum([v.shape[0] for v in vs])].astype(np.int64)
        engine.scene_calib_road(np.array(es, dtype=np.int32), ro, np.concatenate(vs), np.array(f0), np.array(sg))

    def _load_windows(self, engine, data, img, shared):
        """WINDOWS: where a scene has one, or the riders share lanes - the load call has taken them then; -> who is inside when, per
        scene (None: no scene has a window, nothing is passed and nothing is masked)"""
        if not (shared or any(d.windowed for d in data)):
            return None
        if not shared:
            engine.scene_calib_windows(img.enter, img.exit)
        return [d.inside for d in data]

    def _bookkeeping(self, engine, data, img, inside):
        """what `evaluate` and `_trajs` need on the host: the objectives of the simulated riders (NaN outside a window) and, per scene,
        who is simulated and how many present (rider, tick) cells they have - length x simulated riders without windows"""
        objectives = [d.traj[: d.length][:, ~d.replayed][:, :, img.feat] for d in data]
        if inside is not None:
            for q, d in enumerate(data):
                objectives[q][~inside[q][:, ~d.replayed]] = np.nan
        cells = np.array([int((d.exit - d.enter)[~d.replayed].sum()) for d in data])
        return dict(engine=engine, lens=img.lens, feat=img.feat, nr=img.nr, roff=img.roff, R=img.R, sets=self.max_sets, sim=[~d.replayed for d in data],
                    nsim=np.array([int((~d.replayed).sum()) for d in data]), cells=cells, inside=inside, objectives=objectives)

    def _trajs(self, ds, states, k):
        """the scenes of parameter set k from the states of one evaluation: [length, simulated riders, n_feat] each (rows the class
        lacks: 0; NaN outside a rider's presence window)"""
        ns, out = states.shape[2], []
        for q, ln in enumerate(ds["lens"]):
            tr = np.zeros((ln, ds["nr"][q], ds["feat"].size))
            for c, f in enumerate(ds["feat"]):
                if f < ns:
                    tr[:, :, c] = states[:ln, k * ds["R"] + ds["roff"][q]: k * ds["R"] + ds["roff"][q + 1], f]
            if ds["inside"] is not None:
                tr[~ds["inside"][q]] = np.nan
            out.append(tr if ds["sim"][q].all() else tr[:, ds["sim"][q]])
        return out

    def _candidates(self, vals):
        return [self._update_params_args_dict(v) for v in vals]

    def _launch(self, ds, args_list, **kw):
        return self._eval(ds, args_list, **kw, **self._road_over(args_list))

    def _errors(self, ds, sums):
        """per-rider sums -> errors: the riders of a scene added in rider order, then the scenes in scene order"""
        if self.error_func is calc_sse_timesteps:
            return _scenes_in_order(_riders_then_scenes(sums[:, :, 0], ds["roff"]))
        with np.errstate(invalid="ignore", divide="ignore"):       # (an empty scene: nan, as np.mean gives)
            mae = _riders_then_scenes(sums[:, :, 1], ds["roff"]) / (ds["cells"] * float(ds["feat"].size))[None, :]
        return _scenes_in_order(mae ** 2)

    def simulate(self, params_vals, test=False):
        """The trajectories of one parameter vector on the training (test) scenes: ([length, simulated riders, n_feat] per scene -
        the state after each tick -, the objectives)."""
        ds = self._dataset(test)
        args = self._update_params_args_dict(np.asarray(params_vals, dtype=float))
        _, states = self._launch(ds, [args], states=True)
        return self._trajs(ds, states, 0), list(ds["objectives"])

    def run(self, params_vals_guess):
        """The calibration by scipy.optimize.fmin, as DownhillSimplexCalibration.run: fmin's full output with the scenes simulated
        at the optimum appended."""
        from scipy.optimize import fmin

        results = list(fmin(objective_function_wrapper, params_vals_guess, (self,), xtol=self.xtol, ftol=self.ftol, full_output=True,
                            maxiter=self.maxiter, disp=bool(self.verbose)))
        self.param_args_opt = self._update_params_args_dict(results[0])
        results.append(self.simulate(results[0]))
        return results

    def test(self, params_vals=None):
        """Error of a parameter vector - by default the one `run` / `run_many` found - on the TEST scenes."""
        if params_vals is None:
            if self.param_args_opt is None:
                raise RuntimeError("no parameters to test: call run() or run_many() first, or pass params_vals")
            params_vals = [self.param_args_opt[k] for k in self.params_keys]
        return float(self.evaluate([params_vals], test=True)[0])

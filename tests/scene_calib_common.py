"""Shared by tests/test_gpu_scene_calib.py and tests/scene_calib_abi_child.py: small closed-loop scenes per vehicle class and
candidate parameter sets that differ in what the class reads in a closed loop."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from cyclistsocialforce_amd.engine import MODEL_IDS, Engine

MODELS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
# Five scenes from crowd() as it is - P = 1, 2, 8, 32 and 32, slot blocks on odd offsets - and a sixth with a SHORT route: crowd()'s
# only stop lies 61 m ahead and T ticks cover 10 m, so its riders never leave the cruise state.  The riders of the sixth scene pass
# a destination 4 m ahead, reach the last leg of their route around tick 40 (twod_dest then reads row 0 of the position ring until
# tick 100, and tick 127 overwrites that row) and brake for the stop 7 m ahead.  With the default parameters the oracle has them on
# the last leg at tick 38 - 75 and braking from tick 38 - 84 (one Bicycle rider at 198) in every class, and arrived at tick 171 - 191
# in every class but the Bicycle and the InvPendulum, which are still braking at tick 200.
N_RIDERS = np.array([1, 2, 5, 17, 32, 4], dtype=np.int32)
T = 200                                                          # > hist_len = 128: the ring wraps within an evaluation
LENGTHS = np.array([T, 0, T - 37, T, 60, T], dtype=np.int32)
SHORT = 5                                                        # the scene with the short route
REACH = (8.0, 25.0, 60.0, 61.0)
SHORT_REACH = (4.0, 7.0)
VDES = 5.0


def crowd(n, seed, box=14.0, reach=REACH):
    """crowd() of tests/test_gpu_small.py - the first destination 8 m ahead, the last a stop - with the distances of the
    destinations as a parameter.  A deliberate copy: that module imports the suite's fixtures and the oracle, which the child
    process of the ABI test does without.  tests/test_scene_calib_host.py holds the copy (and ORACLE_CASES below) to the original."""
    rng = np.random.default_rng(seed)
    x, y = rng.uniform(0, box, n), rng.uniform(0, box, n)
    psi, v = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    reach = np.asarray(reach, dtype=np.float64)
    m = reach.size + 1
    dq = np.zeros((n, m, 3))
    dq[:, 0, 0], dq[:, 0, 1] = x, y
    dq[:, 1:, 0] = x[:, None] + reach[None, :] * np.cos(psi)[:, None]
    dq[:, 1:, 1] = y[:, None] + reach[None, :] * np.sin(psi)[:, None]
    dq[:, m - 1, 2] = 1.0
    return x, y, psi, v, np.arange(n + 1) * m, dq.reshape(-1, 3)


def field_sets(model, n=7):
    """n parameter sets of one class, built as calib_common.pod_sets builds its own: the default and n - 1 that differ in the
    field (f_0, sigma_0, sigma_2, e_0; the Bicycle's p_0, p_decay), the field of view, the controller gains and the Bicycle's
    v_max_riding"""
    base = parameters.default_pod(model)
    sets = []
    for k in range(n):
        p = _ffi.Params.from_buffer_copy(base)
        p.f_0 = base.f_0 * (1.0 + 0.15 * k)
        p.sigma_0 = base.sigma_0 * (1.0 + 0.05 * k)
        p.sigma_2 = base.sigma_2 * (1.0 - 0.04 * k)
        p.e_0 = base.e_0 * (1.0 - 0.03 * k)
        p.p_0 = base.p_0 * (1.0 + 0.1 * k)
        p.p_decay = base.p_decay * (1.0 + 0.05 * k)
        p.hfov = base.hfov * (1.0 - 0.06 * k)
        p.k_p_v = base.k_p_v * (1.0 + 0.07 * k)
        p.k_p_delta = base.k_p_delta * (1.0 - 0.05 * k)
        p.k_psi = base.k_psi * (1.0 + 0.1 * k)
        if model == "bicycle":
            p.v_max_riding[1] = base.v_max_riding[1] * (1.0 + 0.05 * k)
        for i in range(10):
            p.br_pole_fun[i] = base.br_pole_fun[i] * (1.0 + 0.02 * k)
        sets.append(p)
    return sets


def scenes(model, n_riders=N_RIDERS, seed=0, short=()):
    """the scenes of a data set: (s0 [R, n_states], dest_offsets [R + 1], dest rows [rows, 3]) of all riders, and the same per scene;
    the scenes listed in `short` get the short route"""
    ns = _ffi.N_STATES[MODEL_IDS[model]]
    per, s_all, rows_all, off_all, rows = [], [], [], [0], 0
    for q, n in enumerate(n_riders):
        n = int(n)
        box = 14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)
        if model == "balancingrider":
            box *= 2.0
        x, y, psi, v, off, dq = crowd(n, seed=100 * seed + 10 * n + q, box=box, reach=SHORT_REACH if q in short else REACH)
        s0 = np.zeros((n, ns))
        s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
        per.append((s0, off, dq))
        s_all.append(s0)
        rows_all.append(dq)
        off_all.extend((off[1:] + rows).tolist())
        rows += dq.shape[0]
    return np.concatenate(s_all), np.array(off_all, dtype=np.int64), np.concatenate(rows_all), per


def twin_scene(pod, s0, off, dq, ticks, vdes=VDES):
    """the existing one-wave path: an engine created with that set steps that scene alone, one csf_step call, csf_record at
    stride 1; returns (states [ticks, n, n_states], destination pointers, one-hot navigation state)"""
    n = s0.shape[0]
    e = Engine(pod, n)
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    e.record(stride=1, capacity=max(ticks, 1), forces=False)
    e.step(ticks)
    S, _ = e.recorded(0, ticks)
    assert e.small_ticks() == ticks
    _, ptr, zn, _ = e.state(with_nav=True)
    e.close()
    return S, np.asarray(ptr), np.asarray(zn).reshape(n, 3)


# ---- the scenes of tests/test_gpu_small.py::test_small_crowds_vs_oracle with n <= 8 riders, for the classes that test holds to 1e-4 x
# extent over 400 free ticks, and three parameter sets: the default and the first two of the `field` list of tests/test_gpu_hetero.py
ORACLE_CASES = [("twod", 8, 0, None), ("twod", 5, 1, None), ("twod", 2, 0, 4.0), ("twod", 1, 0, None), ("invpend", 6, 0, None),
                ("planarpoint", 8, 1, 2.0), ("planarpoint", 3, 0, None), ("bicycle", 7, 0, None)]
ORACLE_TICKS = 200


def oracle_fields(model):
    if model == "bicycle":
        return [dict(), dict(hfov=1.2 * np.pi, p_0=40.0, p_decay=4.0), dict(hfov=1.0, p_decay=6.0, k_p_v=13.0)]
    field = [dict(), dict(hfov=1.2 * np.pi, f_0=10.0, sigma_0=0.6, sigma_1=5.5), dict(hfov=1.0, e_0=0.9, e_1=0.4, sigma_2=0.25, sigma_3=4.0)]
    if model == "planarpoint":
        field[2]["poles"] = [-3.0 + 0j]
    return field


def oracle_case(model, n, rule, hfov):
    """(s0, dest_offsets, dest rows, the three csf_params) of one case: the scene as test_small_crowds_vs_oracle builds it"""
    x, y, psi, v, off, dq = crowd(n, seed=10 * n + rule, box=14.0)
    s0 = np.zeros((n, _ffi.N_STATES[MODEL_IDS[model]]))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    over = {} if hfov is None else {"hfov": hfov}
    pods = [parameters.default_pod(model, priority_rule=rule, **{**over, **f}) for f in oracle_fields(model)]
    return s0, off, dq, pods


def oracle_run(pod, s0, off, dq, ticks=ORACLE_TICKS, stride=10):
    """orc.Population free for `ticks` ticks: positions [ticks // stride, n, 2] after every stride-th tick"""
    from oracle import csf_oracle as orc
    pop = orc.Population(orc.Params.from_buffer_copy(bytes(pod)), s0, 5.0, off, dq)
    out = []
    for _ in range(ticks // stride):
        pop.step(stride)
        out.append(pop.state()[:, :2].copy())
    return np.array(out)

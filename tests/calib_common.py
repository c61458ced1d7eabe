"""Shared by tests/test_gpu_calib.py and tests/calib_abi_child.py: a small synthetic calibration data set per vehicle class."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from cyclistsocialforce_amd.engine import Engine

MODELS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
LENGTHS = np.array([300, 217, 0, 120, 263], dtype=np.int32)       # unequal, one sequence empty
T = 300


def pod_sets(model, n=7):
    """n parameter sets of one class: the default and n - 1 that differ in k_p_v / k_p_delta / k_psi / l, as the class has them"""
    base = parameters.default_pod(model)
    sets = []
    for k in range(n):
        p = _ffi.Params.from_buffer_copy(base)
        p.k_p_v = base.k_p_v * (1.0 + 0.07 * k)
        p.k_p_delta = base.k_p_delta * (1.0 - 0.05 * k)
        p.k_psi = base.k_psi * (1.0 + 0.1 * k)
        if model in ("twod", "bicycle", "invpend", "planarbike"):
            p.l = base.l * (1.0 + 0.03 * k)
        for i in range(10):                      # (the BalancingRider's yaw loop: pole functions and fixed gains)
            p.br_pole_fun[i] = base.br_pole_fun[i] * (1.0 + 0.02 * k)
        for i in range(5):
            p.br_gains[i] = base.br_gains[i] * (1.0 + 0.02 * k)
        sets.append(p)
    return sets


def data_set(model, seed=0, n_seq=5, ticks=T):
    """start states [n_seq, n_states], forces Fx, Fy [ticks, n_seq]: a speed of 3 .. 5 m/s along a slowly turning direction"""
    rng = np.random.default_rng(seed)
    ns = _ffi.N_STATES[Engine_model_id(model)]
    s0 = np.zeros((n_seq, ns))
    s0[:, 0], s0[:, 1] = rng.uniform(-20, 20, n_seq), rng.uniform(-20, 20, n_seq)
    s0[:, 2] = rng.uniform(-np.pi, np.pi, n_seq)
    s0[:, 3] = rng.uniform(3.0, 5.0, n_seq)
    t = np.arange(ticks)[:, None] * 0.01
    phi = s0[None, :, 2] + rng.uniform(0.2, 0.6, n_seq)[None, :] * np.sin(rng.uniform(0.5, 1.5, n_seq)[None, :] * t + rng.uniform(0, 6, n_seq)[None, :])
    mag = 4.0 + rng.uniform(0.2, 1.0, n_seq)[None, :] * np.sin(0.8 * t + rng.uniform(0, 6, n_seq)[None, :])
    return s0, mag * np.cos(phi), mag * np.sin(phi)


def Engine_model_id(model):
    from cyclistsocialforce_amd.engine import MODEL_IDS
    return MODEL_IDS[model]


def twin_states(model, sets, s0, Fx, Fy, lengths, fix_speed, stride):
    """the existing path: one engine holding every (set, sequence) as a road user with its parameter set, csf_replay_forces"""
    k, n_seq = len(sets), s0.shape[0]
    e = Engine(sets[0], k * n_seq)
    e.add_agents(np.tile(s0, (k, 1)), 0.0)
    e.set_param_classes(sets, cls=np.repeat(np.arange(k), n_seq))
    out = e.replay_forces(np.tile(Fx, (1, k)), np.tile(Fy, (1, k)), lengths=None if lengths is None else np.tile(lengths, k),
                          fix_speed=fix_speed, stride=stride)
    e.close()
    return out

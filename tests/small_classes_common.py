"""Shared by tests/test_gpu_small_classes.py, tests/test_small_classes_host.py and tests/small_classes_abi_child.py: small
populations of several parameter sets and vehicle classes - the UncontrolledVehicle's among them -, built as a stepping engine holds them
(csf_set_param_classes, csf_set_agent_class, csf_set_script), with the switch of csf_small_classes on or off.  The twin of a population is
the same population with the switch off: the general path."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from scene_calib_common import VDES, crowd, field_sets
from scene_groups_common import GENERAL_TOL  # noqa: F401  (the bar of the one-wave tick against the general path: see there)
from scene_mixed_common import mixed_sets

RIDERS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
TICKS = 40

# The seeds of the crowds: chosen with the CPU oracle so that no population is chaotic over the test's ticks - a start moved by 1e-7 m
# stays within a tenth of the bound (tests/test_small_classes_host.py::test_the_oracle_is_not_chaotic_on_the_cases).
SEED_A, BOX_A = 914, 6.0           # (a): two TwoD riders of two sets - scene_groups_common's ACT scene of 2
SEED_B, BOX_B = 3051, 14.0         # (b): five riders twod, bicycle, bicycle, invpend, twod - scene_mixed_common's scene of 5
SEED_C, BOX_C = 3359, 30.0         # (c): 32 riders round robin over the six rider classes, in the 30 m box
SEED_D, BOX_D = 324, 30.0          # (d): 32 TwoD riders, 32 sets
SEED_E, BOX_E = 3033, 14.0         # (e): four cyclists and a scripted car
SEED_F, BOX_F = 3014, 14.0         # (f): one rider of set 1


def wide(x, y, psi, v, ns):
    s0 = np.zeros((len(x), ns))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    return s0


def car_script(x0, y0, psi, v, rows=64, t_s=0.01):
    """the prescribed trajectory of an UncontrolledVehicle (vehicle.py:958-960): rows (x, y, psi, v) of a straight line"""
    t = np.arange(rows) * t_s
    return np.c_[x0 + v * t * np.cos(psi), y0 + v * t * np.sin(psi), np.full(rows, psi), np.full(rows, v)]


def case(name, rule=0):
    """a population: dict(pods, cls, s0 [n, ns], off, dq, script = None | (idx, offsets, rows), box)"""
    def with_rule(pods):
        out = []
        for p in pods:
            q = _ffi.Params.from_buffer_copy(bytes(p))
            q.priority_rule = rule
            out.append(q)
        return out

    script = None
    if name == "a":
        x, y, psi, v, off, dq = crowd(2, seed=SEED_A, box=BOX_A)
        base = parameters.default_pod("twod")
        pods, cls, box = [base, parameters.default_pod("twod", f_0=base.f_0 * 1.6, hfov=2.0)], [0, 1], BOX_A
    elif name == "b":
        x, y, psi, v, off, dq = crowd(5, seed=SEED_B, box=BOX_B)
        pods, cls, box = list(mixed_sets()[0][:3]), [0, 1, 1, 2, 0], BOX_B
    elif name == "c":
        x, y, psi, v, off, dq = crowd(32, seed=SEED_C, box=BOX_C)
        pods, cls, box = list(mixed_sets()[0]), list(np.arange(32) % 6), BOX_C
    elif name == "d":
        x, y, psi, v, off, dq = crowd(32, seed=SEED_D, box=BOX_D)
        flat = field_sets("twod", 7)
        pods = []
        for k in range(32):                                        # 32 distinct sets: seven fields x five scalings of f_0 and the field of view
            p = _ffi.Params.from_buffer_copy(flat[k % 7])
            p.f_0 *= 1.0 + 0.03 * (k // 7)
            p.hfov *= 1.0 - 0.02 * (k // 7)
            p.v_max_riding[1] *= 1.0 + 0.01 * k
            pods.append(p)
        cls, box = list(range(32)), BOX_D
    elif name == "e":
        x, y, psi, v, off, dq = crowd(5, seed=SEED_E, box=BOX_E)
        x[4], y[4], psi[4], v[4] = -1.0, 0.5 * BOX_E, 0.0, 6.0      # the car crosses the box from the left
        dq = dq.copy()
        dq[off[4]: off[5], 0] = x[4] + np.array([0.0, 8.0, 25.0, 60.0, 61.0])
        dq[off[4]: off[5], 1] = y[4]
        pods = [parameters.default_pod("twod"), parameters.default_pod("uncontrolled", hfov=2.5, f_0=9.0)]
        cls, box = [0, 0, 0, 0, 1], BOX_E
        script = (np.array([4]), np.array([0, 64]), car_script(x[4], y[4], psi[4], v[4]))
    elif name == "f":
        x, y, psi, v, off, dq = crowd(1, seed=SEED_F, box=BOX_F)
        pods, cls, box = [parameters.default_pod("twod"), parameters.default_pod("twod", hfov=1.2, f_0=10.0, k_p_v=12.0)], [1], BOX_F
    else:
        raise KeyError(name)
    pods = with_rule(pods)
    ns = max(_ffi.N_STATES[p.model] for p in pods)
    return dict(pods=pods, cls=np.array(cls, dtype=np.int32), s0=wide(x, y, psi, v, ns), off=off, dq=dq, script=script, box=box)


def build(c, on, capacity=None, road=None):
    """the population on an Engine, csf_small_classes(on)"""
    from cyclistsocialforce_amd.engine import Engine
    n = c["s0"].shape[0]
    e = Engine(c["pods"][0], capacity or n)
    e.small_classes(on)
    e.set_param_classes(c["pods"])                                 # (before the road users: the widest state from here on)
    e.add_agents(c["s0"], VDES)
    e.set_dest_queue(np.arange(n), c["off"], c["dq"], reset=True)
    e.set_agent_class(np.arange(n), c["cls"])
    if c["script"] is not None:
        e.set_script(*c["script"])
    if road is not None:
        e.set_road(*road)
    return e


def unc_population(n=6, seed=6):
    """n UncontrolledVehicles with scripts of 100 rows (tests/test_gpu_batch.py's "unc" member): one set, no rider class"""
    x, y, psi, v, off, dq = crowd(n, seed=seed)
    rows = np.concatenate([car_script(x[j], y[j], psi[j], v[j], rows=100) for j in range(n)])
    return dict(pods=[parameters.default_pod("uncontrolled")], cls=np.zeros(n, dtype=np.int32), s0=wide(x, y, psi, v, 4), off=off, dq=dq,
                script=(np.arange(n), np.arange(n + 1) * 100, rows), box=14.0)


def single_population(n=5, seed=77, model="twod"):
    x, y, psi, v, off, dq = crowd(n, seed=seed)
    pod = parameters.default_pod(model)
    return dict(pods=[pod], cls=np.zeros(n, dtype=np.int32), s0=wide(x, y, psi, v, _ffi.N_STATES[pod.model]), off=off, dq=dq, script=None, box=14.0)


def oracle_population(c):
    """orc.Population of a case (set_classes), in the layout as wide as the engine's"""
    from oracle import csf_oracle as orc
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in c["pods"]]
    ns = c["s0"].shape[1]
    pop = orc.Population(classes[0], c["s0"], VDES, c["off"], c["dq"], ns=ns)
    pop.set_classes(classes, np.asarray(c["cls"], dtype=np.uint8))
    return pop


def lacking_rows(c):
    """[n, ns] bool: the state rows the class of every road user lacks (they stay exactly 0)"""
    ns = c["s0"].shape[1]
    width = np.array([_ffi.N_STATES[c["pods"][k].model] for k in c["cls"]])
    return np.arange(ns)[None, :] >= width[:, None]


# ---- the oracle case of test 4: scene_mixed_common.oracle_case - 5 riders twod / bicycle / invpend, both priority rules; its seed is held by
# tests/test_scene_mixed_host.py and, for the population as THIS path holds it, by tests/test_small_classes_host.py
def oracle_case(rule, k=0):
    from scene_mixed_common import ORACLE_GROUP, oracle_case as mixed_case
    s0, off, dq, pods = mixed_case(rule)
    return dict(pods=list(pods[k]), cls=np.array(ORACLE_GROUP, dtype=np.int32), s0=s0[:, :6].copy(), off=off, dq=dq, script=None, box=14.0)


# ---- test 5: which rider owns which of two sets.  Case (a) with the sets swapped between the two riders: both riders move by well over
# SWAP_MOVED within TICKS ticks (the CPU oracle: tests/test_small_classes_host.py::test_a_swap_of_the_sets_moves_the_riders)
SWAP_MOVED = 1e-2

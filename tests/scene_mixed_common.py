"""Shared by tests/test_gpu_scene_mixed.py, tests/test_scene_mixed_host.py and tests/scene_mixed_abi_child.py: small
closed-loop scenes whose riders are of several vehicle classes, candidates of one parameter set per group - every group of a class of its
own -, and the oracle run with them.  The general-path twin is scene_groups_common.general_twin: it takes records of any class."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from cyclistsocialforce_amd.engine import MODEL_IDS
from scene_calib_common import VDES, crowd, field_sets
from scene_groups_common import GENERAL_TOL  # noqa: F401  (the bar of the one-wave tick against the general path: see there)

# group g is of class CLASSES[g]: record 0 is a TwoD's, group 1 the Bicycle's - the class with the field of its own
CLASSES = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
MODELS = np.array([MODEL_IDS[m] for m in CLASSES], dtype=np.int32)
G = len(CLASSES)
WIDTH = 8                                                       # the widest state: the BalancingRider's
# scene            a          b                c: P = 32, all six        d: group 1 only     e       f: empty    g: 25 < T
N_RIDERS = np.array([2, 5, 32, 3, 1, 4, 25], dtype=np.int32)
T = 40
LENGTHS = np.array([T, T, T, T, T, 0, 25], dtype=np.int32)
GROUPS = [np.array([0, 2]), np.array([0, 1, 1, 2, 0]), np.arange(32) % 6, np.array([1, 1, 1]), np.array([2]), np.array([0, 1, 2, 3]),
          (np.arange(25) + 3) % 6]
GROUP = np.concatenate(GROUPS).astype(np.uint8)
ROFF = np.r_[0, np.cumsum(N_RIDERS)]
R = int(ROFF[-1])
# crowd(n, SEEDS[q], BOXES[q]): the seeds are chosen with the CPU oracle so that no scene is chaotic over its ticks
# (tests/test_scene_mixed_host.py::test_the_mixed_oracle_is_not_chaotic_on_the_scenes).  The scenes with a BalancingRider get the wider
# box scene_calib_common.scenes gives that class.
SEEDS = (3020, 3051, 3359, 3033, 3014, 3045, 3256)
BOXES = (14.0, 14.0, 60.0, 14.0, 14.0, 14.0, 60.0)


def wide_state(x, y, psi, v):
    s0 = np.zeros((len(x), WIDTH))
    s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3] = x, y, psi, v
    return s0


def mixed_scenes(n_riders=N_RIDERS, seeds=SEEDS, boxes=BOXES):
    """(s0 [R, 8], dest_offsets [R + 1], dest rows) of all riders, and the same per scene"""
    per, s_all, rows_all, off_all, rows = [], [], [], [0], 0
    for n, seed, box in zip(n_riders, seeds, boxes):
        x, y, psi, v, off, dq = crowd(int(n), seed=seed, box=box)
        s0 = wide_state(x, y, psi, v)
        per.append((s0, off, dq))
        s_all.append(s0)
        rows_all.append(dq)
        off_all.extend((off[1:] + rows).tolist())
        rows += dq.shape[0]
    return np.concatenate(s_all), np.array(off_all, dtype=np.int64), np.concatenate(rows_all), per


def mixed_sets(n_sets=3, classes=CLASSES):
    """n_sets candidates of one record per group, record g of class classes[g]: the records differ in the field (f_0, sigma, e; the
    Bicycle's p_0, p_decay), the field of view, the gains (field_sets) and v_max_riding; candidate 1 has the second priority rule"""
    flat = {m: field_sets(m, 7) for m in set(classes)}
    out = []
    for k in range(n_sets):
        tup = []
        for g, m in enumerate(classes):
            p = _ffi.Params.from_buffer_copy(flat[m][(3 * g + k) % 7])
            p.v_max_riding[1] = p.v_max_riding[1] * (1.0 + 0.04 * g)
            p.priority_rule = 1 if k == 1 else 0
            tup.append(p)
        out.append(tuple(tup))
    return out


def oracle_mixed_run(pods, grp, s0, off, dq, ticks, stride=1, rows=2):
    """orc.Population with one parameter set per group, of any class (set_classes), free for `ticks` ticks: the first `rows` state rows
    [ticks // stride, n, rows] in the layout as wide as the widest class of `pods`"""
    from oracle import csf_oracle as orc
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in pods]
    ns = max(_ffi.N_STATES[p.model] for p in pods)
    pop = orc.Population(classes[0], s0[:, :ns], VDES, off, dq, ns=ns)
    pop.set_classes(classes, np.asarray(grp, dtype=np.uint8))
    out = []
    for _ in range(ticks // stride):
        pop.step(stride)
        out.append(pop.state()[:, :rows].copy())
    return np.array(out)


# ---- the oracle case: 5 riders of three classes (twod, bicycle, invpend), both priority rules, three candidates; crowd(5, ORACLE_SEED) of
# the 14 m box, the seed chosen on the CPU (tests/test_scene_mixed_host.py::test_the_mixed_oracle_is_not_chaotic_on_the_horizon)
ORACLE_SEED = 51
ORACLE_TICKS = 200
ORACLE_CLASSES = ("twod", "bicycle", "invpend")
ORACLE_GROUP = np.array([0, 1, 2, 0, 1], dtype=np.uint8)
ORACLE_FIELDS = [(dict(), dict(hfov=1.2 * np.pi, p_0=40.0, p_decay=4.0), dict(f_0=10.0, sigma_0=0.6)),
                 (dict(hfov=1.2 * np.pi, f_0=10.0, sigma_0=0.6, sigma_1=5.5), dict(hfov=1.0, p_decay=6.0, k_p_v=13.0), dict(hfov=1.0, e_0=0.9, e_1=0.4)),
                 (dict(hfov=4.0), dict(), dict(hfov=2.0, f_0=7.0, k_p_v=12.0))]


def oracle_case(rule):
    x, y, psi, v, off, dq = crowd(5, seed=ORACLE_SEED, box=14.0)
    pods = [tuple(parameters.default_pod(m, priority_rule=rule, **f) for m, f in zip(ORACLE_CLASSES, trio)) for trio in ORACLE_FIELDS]
    return wide_state(x, y, psi, v), off, dq, pods


# ---- the scene on which the classes ACT: two riders, one a Bicycle and one a TwoD; swapping which of the two is the Bicycle changes both
# trajectories.  Seed and threshold by the CPU oracle (tests/test_scene_mixed_host.py::test_the_classes_act_on_the_seeded_scene).
ACT_SEED, ACT_BOX, ACT_TICKS, ACT_MOVED = 914, 6.0, 40, 1e-2


def act_scene():
    x, y, psi, v, off, dq = crowd(2, seed=ACT_SEED, box=ACT_BOX)
    return wide_state(x, y, psi, v), off, dq


def act_pods():
    return parameters.default_pod("twod"), parameters.default_pod("bicycle")


# ---- the scene of the tests with the other hooks (replay, windows, road): 8 riders - Bicycles, InvPendulums, a BalancingRider and a TwoD;
# the seed by the CPU oracle as SEEDS
HOOK_CLASSES = ("bicycle", "invpend", "balancingrider", "twod")
HOOK_GROUP = np.array([0, 1, 2, 3, 0, 1, 0, 1], dtype=np.uint8)
HOOK_SEED, HOOK_BOX = 3256, 40.0

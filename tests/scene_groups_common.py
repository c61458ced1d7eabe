"""Shared by tests/test_gpu_scene_groups.py and tests/test_scene_groups_host.py: small closed-loop scenes whose
riders are in groups, candidate sets of one parameter set per group, the general-path twin that holds per-vehicle parameter sets, and
the oracle run with them."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from scene_calib_common import VDES, crowd, field_sets, scenes

MODELS = ("twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider")
# riders | groups present | assignment | length: 2 riders, one of each; 5 mixed; a full wave of 32 (P = 32, two source groups of lanes)
# round robin over four groups; 3 riders all in group 0; a single rider (of group 1: nobody carries group 0's set); an empty scene
N_RIDERS = np.array([2, 5, 32, 3, 1, 4], dtype=np.int32)
T = 40
LENGTHS = np.array([T, 25, T, T, T, 0], dtype=np.int32)
G = 4
GROUPS = [np.array([0, 1]), np.array([0, 1, 1, 0, 1]), np.arange(32) % 4, np.zeros(3, dtype=int), np.array([1]), np.array([0, 1, 2, 1])]
GROUP = np.concatenate(GROUPS).astype(np.uint8)
ROFF = np.r_[0, np.cumsum(N_RIDERS)]
R = int(ROFF[-1])
# The scenes are scene_calib_common.scenes(model, N_RIDERS, seed=SCENE_SEED): crowd(n, 100 * SCENE_SEED + 10 n + q).  The seed is chosen
# with the CPU oracle (tests/test_scene_groups_host.py::test_the_groups_act_on_the_seeded_scenes): in the scenes of 2 and of 5 TwoD riders
# another f_0 for group 1 moves EVERY rider by far more than rounding within the scene's ticks.
SCENE_SEED = 3
GENERAL_TOL = 2e-5          # tests/test_gpu_small.py::test_general_path_agrees_and_is_taken_when_asked: one-wave tick against the
                            # general path, positions after 300 ticks; here over at most 40 ticks, on every state row


def group_scenes(model):
    return scenes(model, N_RIDERS, seed=SCENE_SEED)


def group_sets(model, n_sets=3, n_groups=G):
    """n_sets candidates of n_groups parameter sets each: the records differ in the field (f_0, sigma, e; the Bicycle's p_0, p_decay), the
    field of view, the gains (field_sets) and v_max_riding; candidate 1 has the second priority rule in every record, and the LAST
    candidate has it in the record of group 1 alone - the rule of a candidate is its first record's"""
    flat = field_sets(model, 7)
    out = []
    for k in range(n_sets):
        tup = []
        for g in range(n_groups):
            p = _ffi.Params.from_buffer_copy(flat[(3 * g + k) % 7])      # (distinct within a candidate)
            p.v_max_riding[1] = p.v_max_riding[1] * (1.0 + 0.04 * g)
            p.priority_rule = 1 if k == 1 else 0
            tup.append(p)
        if k == n_sets - 1 and n_groups > 1:
            tup[1].priority_rule = 1
        out.append(tuple(tup))
    return out


def general_twin(pods, grp, s0, off, dq, ticks, enter=None, exit=None, replayed=None, rec=None, road=None, vdes=VDES):
    """The engine's general path - a pair launch and a per-agent launch per tick, which an engine with several parameter sets always
    takes - for one (candidate, scene): an Engine created with the candidate's first record (its priority rule is the intersection's)
    holds all records as parameter classes and every rider the class of its group, and is stepped in 1-tick calls.  Windows, replay
    and road as tests/scene_windows_common.py::window_twin and scene_road_common.twin_road have them.  Returns the states
    [ticks, n, n_states] after every tick (NaN where a rider is absent)."""
    from cyclistsocialforce_amd.engine import Engine
    n = s0.shape[0]
    enter = np.zeros(n, dtype=int) if enter is None else enter
    exit = np.full(n, ticks, dtype=int) if exit is None else exit
    e = Engine(pods[0], n)
    e.set_param_classes(list(pods) if len(pods) > 1 else [pods[0], pods[0]])
    if road is not None:
        e.set_road(*road)
    vd = np.broadcast_to(np.asarray(vdes, dtype=float), (n,))
    ids = []
    out = np.full((ticks, n, e.ns), np.nan)
    for t in range(ticks):
        gone = [k for k, r in enumerate(ids) if exit[r] == t]
        if gone:
            e.remove_agents(gone)
            ids = [r for r in ids if exit[r] != t]
        new = [r for r in range(n) if enter[r] == t and exit[r] > t]
        if new:
            e.add_agents(s0[new], vd[new])
            where = np.arange(len(ids), len(ids) + len(new))
            e.set_agent_class(where, np.asarray(grp)[new])
            rows = [dq[off[r]: off[r + 1]] for r in new]
            e.set_dest_queue(where, np.r_[0, np.cumsum([len(x) for x in rows])], np.concatenate(rows), reset=True)
            ids += new
        if not ids:
            continue
        e.step(1)
        s = e.state()
        if replayed is not None:
            idx = np.array([k for k, r in enumerate(ids) if replayed[r]], dtype=np.int32)
            if idx.size:
                s[idx, :4] = rec[t, [ids[k] for k in idx], :4]
                e.push_state(idx, s[idx])
        out[t, ids] = s
    assert e.small_ticks() == 0                                  # (several parameter sets: never the one-wave tick)
    e.close()
    return out


# ---- the oracle case: TwoD, 5 riders, two groups, both priority rules; three candidates whose groups differ in the field, the field of
# view and v_max_riding.  The crowd is crowd(5, ORACLE_SEED) of tests/test_gpu_small.py's 14 m box; the seed is chosen on the CPU so that
# the oracle is not chaotic over ORACLE_TICKS (tests/test_scene_groups_host.py::test_the_grouped_oracle_is_not_chaotic_on_the_horizon).
ORACLE_SEED = 51
ORACLE_TICKS = 200
ORACLE_GROUP = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
ORACLE_FIELDS = [(dict(), dict(f_0=10.0, sigma_0=0.6, hfov=1.2 * np.pi)),
                 (dict(hfov=1.2 * np.pi, f_0=10.0, sigma_0=0.6, sigma_1=5.5), dict(hfov=1.0, e_0=0.9, e_1=0.4, sigma_2=0.25, sigma_3=4.0)),
                 (dict(hfov=4.0), dict(hfov=2.0, f_0=7.0, v_max_riding=(5.0, 6.0)))]


def oracle_case(rule):
    x, y, psi, v, off, dq = crowd(5, seed=ORACLE_SEED, box=14.0)
    s0 = np.c_[x, y, psi, v, np.zeros(5)]
    pods = [tuple(parameters.default_pod("twod", priority_rule=rule, **f) for f in pair) for pair in ORACLE_FIELDS]
    return s0, off, dq, pods


def oracle_group_run(pods, grp, s0, off, dq, ticks=ORACLE_TICKS, stride=10):
    """orc.Population with one parameter set per group (set_classes), free for `ticks` ticks: positions [ticks // stride, n, 2]"""
    from oracle import csf_oracle as orc
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in pods]
    pop = orc.Population(classes[0], s0, VDES, off, dq)
    pop.set_classes(classes, np.asarray(grp, dtype=np.uint8))
    out = []
    for _ in range(ticks // stride):
        pop.step(stride)
        out.append(pop.state()[:, :2].copy())
    return np.array(out)


# ---- the scenes on which the groups ACT: two TwoD crowds of tests/test_gpu_small.py's kind in small boxes, seeds chosen with the CPU
# oracle so that f_0 x 1.6 in group 1 alone moves EVERY rider within 40 ticks - the least affected one by 1.2e-2 m (2 riders) and
# 8.6e-3 m (5 riders); tests/test_scene_groups_host.py::test_the_groups_act_on_the_seeded_scenes holds the choice to 1e-4 m.
ACT_SCENES = ((2, 914, 6.0, np.array([0, 1], dtype=np.uint8)), (5, 975, 8.0, np.array([0, 1, 1, 0, 1], dtype=np.uint8)))
ACT_TICKS = 40
ACT_F0 = 1.6


def act_scene(k):
    n, seed, box, grp = ACT_SCENES[k]
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    return np.c_[x, y, psi, v, np.zeros(n)], off, dq, grp


def act_pods():
    base = parameters.default_pod("twod")
    return base, parameters.default_pod("twod", f_0=base.f_0 * ACT_F0)

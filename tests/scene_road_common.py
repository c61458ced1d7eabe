"""Shared by tests/test_gpu_scene_road.py, tests/test_scene_road_host.py and tests/scene_road_abi_child.py: closed-loop scenes
with road edges - one data set whose roads sit where the staging, the padding, the tiles and the limits of the
one-wave tick can go wrong -, twins with a road, and the oracle cases between two road edges."""
import numpy as np

from scene_calib_common import ORACLE_TICKS, SHORT_REACH, VDES, crowd, field_sets, oracle_case, scenes  # noqa: F401

# scene      a  b  c  d  e   f (the short route of scene_calib_common)
N_RIDERS = np.array([1, 2, 5, 8, 32, 4], dtype=np.int32)
T = 40
LENGTHS = np.array([25, T, 33, T, T, T], dtype=np.int32)
SHORT = 5
# vertices of the road of every scene and the sigma of its edges (None: no road):
#   b  64 = one block of 64, one edge                    c  65: nv_pad 128, 63 inert vertices
#   d  2 048 = SMALL_ROAD_MAX in two edges with different integer sigmas: two tiles of 1 024, road_np = 0
#   e  512 with 32 riders: nv_pad x P = 16 384, the limit; sigma 2.5: the exp2 / log2 form
#   f  1 100: a partial second tile, nv_pad 1 152
ROADS = (None, ((64,), (2.0,)), ((65,), (2.0,)), ((1024, 1024), (2.0, 3.0)), ((256, 256), (2.5, 2.5)), ((550, 550), (3.0, 3.0)))
# Strengths of the first and the second edge.  The reference's default F_0 = 0.05 moves a rider 10 m from an edge by nanometres in
# 40 ticks; these make every rider of every roaded scene move by more than 1e-4 m against the same scene without a road on the
# CPU oracle (tests/test_scene_road_host.py::test_the_road_acts_on_the_oracle holds them to it).
F0_EDGES = (6.0, 9.0)
# (set k: F_0, sigma) of the override test: integer sigmas 1 .. 5 (the powers of rsq), fractional ones (exp2 / log2), and F_0 = 0
OVERRIDES = ((4.0, 2.0), (7.5, 2.5), (0.0, 3.0), (5.0, 1.0), (12.0, 4.0), (3.0, 3.7), (20.0, 5.0))
ZERO_SET = 2


def box_of(model, n):
    box = 14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)
    return 2.0 * box if model == "balancingrider" else box


def road_of(model, q, f0=None, sigma=None):
    """the road of scene q as Engine.set_road takes it - polylines beside the box of the scene's crowd, the first below it and the
    second above, as tests/test_gpu_batch.py builds its roads - or None; f0 / sigma: one value for every edge instead of the scene's"""
    if ROADS[q] is None:
        return None
    counts, sigmas = ROADS[q]
    box = box_of(model, int(N_RIDERS[q]))
    ys = (-3.0, box + 3.0)
    verts = np.concatenate([np.c_[np.linspace(-20.0, box + 20.0, c), np.full(c, ys[k])] for k, c in enumerate(counts)])
    F0 = np.array(F0_EDGES[: len(counts)]) if f0 is None else np.full(len(counts), float(f0))
    sg = np.array(sigmas) if sigma is None else np.full(len(counts), float(sigma))
    return np.r_[0, np.cumsum(counts)].astype(np.int64), verts, F0, sg


def road_args(model, drop=()):
    """(edge_scene, offsets, verts, F0, sigma) of the data set's roads as Engine.scene_calib_road takes them"""
    es, off, vs, f0, sg = [], [0], [], [], []
    for q in range(len(N_RIDERS)):
        r = road_of(model, q)
        if r is None or q in drop:
            continue
        for k in range(r[0].size - 1):
            es.append(q)
            vs.append(r[1][r[0][k]: r[0][k + 1]])
            off.append(off[-1] + vs[-1].shape[0])
            f0.append(r[2][k])
            sg.append(r[3][k])
    return np.array(es, dtype=np.int32), np.array(off, dtype=np.int64), np.concatenate(vs), np.array(f0), np.array(sg)


def rule_sets(model, rule, n=7):
    sets = field_sets(model, n)
    for p in sets:
        p.priority_rule = rule
    return sets


def twin_road(pod, s0, off, dq, ticks, road, vdes=VDES):
    """scene_calib_common.twin_scene with a road: a stand-alone engine that holds the scene and its road (set_road), stepped by the
    one-wave tick in one csf_step call; (states [ticks, n, n_states], destination pointers, one-hot navigation state)"""
    from cyclistsocialforce_amd.engine import Engine
    n = s0.shape[0]
    e = Engine(pod, n)
    e.add_agents(s0, vdes)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    if road is not None:
        e.set_road(*road)
    e.record(stride=1, capacity=max(ticks, 1), forces=False)
    e.step(ticks)
    S, _ = e.recorded(0, ticks)
    assert e.small_ticks() == ticks
    _, ptr, zn, _ = e.state(with_nav=True)
    e.close()
    return S, np.asarray(ptr), np.asarray(zn).reshape(n, 3)


def oracle_road_run(pod, s0, off, dq, road, ticks, stride=10):
    """orc.Population with set_road, free for `ticks` ticks: positions [ticks // stride, n, 2] after every stride-th tick"""
    from oracle import csf_oracle as orc
    pop = orc.Population(orc.Params.from_buffer_copy(bytes(pod)), s0, 5.0, off, dq)
    if road is not None:
        pop.set_road(*road)
    out = []
    for _ in range(ticks // stride):
        pop.step(stride)
        out.append(pop.state()[:, :2].copy())
    return np.array(out)


# ---- the oracle cases: one TwoD (the second priority rule), one Bicycle and one PlanarPoint case of scene_calib_common.ORACLE_CASES,
# each between two road edges of 700 vertices as tests/test_gpu_small.py::test_small_crowds_between_road_edges_vs_oracle places them -
# but 13 m beside the box of 14 m: in the 200 ticks compared a rider covers up to 12 m, and an edge it crossed would put it within
# centimetres of a vertex, where r^-(sigma+1) makes any run chaotic.  The strengths are raised accordingly.
ORACLE_ROAD_CASES = [("twod", 5, 1, None), ("bicycle", 7, 0, None), ("planarpoint", 3, 0, None)]


def oracle_road():
    xs = np.linspace(-20.0, 50.0, 700)
    verts = np.r_[np.c_[xs, np.full(700, -13.0)], np.c_[xs, np.full(700, 27.0)]]
    return np.array([0, 700, 1400], dtype=np.int64), verts, np.array([15.0, 20.0]), np.array([2.0, 2.0])


# ---- the recovery: 8 scenes of 3 - 5 riders x 60 ticks between two edges 4 m beside the box of 10 m (60 ticks cover at most 3.6 m);
# sigma is RoadElementParameters()'s, which a fit of road_F_0 alone keeps
RECOVERY_N = (3, 4, 5, 3, 4, 5, 3, 4)
RECOVERY_TICKS = 60


def recovery_scene(q):
    n = RECOVERY_N[q]
    x, y, psi, v, off, dq = crowd(n, seed=700 + q, box=10.0)
    s0 = np.c_[x, y, psi, v, np.zeros(n)]
    xs = np.linspace(-15.0, 25.0, 200)
    verts = np.r_[np.c_[xs, np.full(200, -4.0)], np.c_[xs, np.full(200, 14.0)]]
    return s0, off, dq, (np.array([0, 200, 400], dtype=np.int64), verts, np.array([0.15, 0.15]), np.array([3.0, 3.0]))

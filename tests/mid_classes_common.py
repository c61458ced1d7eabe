"""Shared by tests/test_gpu_mid_classes.py, tests/test_mid_classes_host.py and tests/mid_classes_abi_child.py: mid-size
populations (33 ... 1 024 road users) of several parameter sets and vehicle classes - scripted UncontrolledVehicles among them -, built as a
stepping engine holds them (csf_set_param_classes, csf_set_agent_class, csf_set_script), with the switch of csf_mid_classes on or off.  The
twin of a population is the same population with the switch off: the general path (a pair launch and a per-agent launch per class)."""
import numpy as np

from cyclistsocialforce_amd import _ffi, parameters
from scene_calib_common import VDES, crowd, field_sets
from small_classes_common import car_script, wide

# The bars (the issue's, which are the project's own in tests/test_gpu_hetero.py::test_random_mixed_population_vs_oracle):
FORCE_TOL = 1e-4                   # total forces of one tick from a common state: x the largest force (twin and oracle)
POS_TOL = 1e-4                     # positions: x box, within a window of WINDOW ticks from a common state (oracle), over 10 one-tick calls (twin)
ROW_TOL = np.array([2e-3, 5e-3, 5e-3, 5e-3])   # headings; speeds, steer and lean angles within a window
WINDOW, TICKS = 10, 50

ORDER = ("twod", "bicycle", "invpend", "planarpoint", "planarbike")
OWN = {"twod": dict(hfov=1.0, f_0=10.0), "bicycle": dict(hfov=3.4, p_0=40.0, p_decay=4.0), "invpend": dict(hfov=2.5, e_0=0.9, k_p_v=12.0, v_max_walk=3.5),
       "planarpoint": dict(hfov=1.5, f_0=5.0, poles=[-3.0 + 0j]), "planarbike": dict(hfov=2.8, sigma_0=0.6)}


def box_for(n):
    """(tests/test_gpu_batch_mid.py: the density of its mid-size members)"""
    return max(30.0, 3.2 * np.sqrt(n))


def twod_sets(k, models=("twod",)):
    """k distinct sets of the TwoD field: seven fields x scalings of f_0, the field of view and the speed limit (small_classes_common, case
    d), dealt over `models` in turn"""
    flat = [field_sets(m, 7) for m in models]
    pods = []
    for i in range(k):
        p = _ffi.Params.from_buffer_copy(flat[i % len(models)][i % 7])
        p.f_0 *= 1.0 + 0.01 * (i // 7)
        p.hfov *= 1.0 - 0.005 * (i // 7)
        p.v_max_riding[1] *= 1.0 + 0.001 * i
        pods.append(p)
    return pods


def five_class_sets():
    """the ten sets of tests/test_gpu_hetero.py::test_random_mixed_population_vs_oracle: five classes, defaults and a set of their own"""
    return [parameters.default_pod(m) for m in ORDER] + [parameters.default_pod(m, **OWN[m]) for m in ORDER]


# (kind, road users, priority rule) -> seed of the crowd.  Chosen with the CPU oracle so that no population is chaotic over a window: a
# start moved by one fp32 ulp of the coordinate bound stays within a tenth of the window's bar
# (tests/test_mid_classes_host.py::test_the_oracle_is_not_chaotic_on_the_seeds).
CASES = [("two", 33, 0), ("two", 40, 1), ("sets", 33, 0), ("five", 65, 1), ("sets", 257, 0), ("five", 257, 1), ("cars", 65, 0), ("five", 600, 0)]
DEAD = (5, 17, 18, 30)             # road users removed again: dead slots in the middle
# ... against the twin over 10 one-tick calls (kind, road users, rule, dead slots), and the forces of one tick with dead slots and poisoned slack
TWIN_CASES = [("two", 33, 0, ()), ("sets", 33, 1, ()), ("five", 65, 0, DEAD), ("cars", 65, 1, ()), ("sets", 257, 1, DEAD), ("five", 257, 0, ()),
              ("five", 600, 1, DEAD)]
DEAD_FORCE_CASES = [("five", 37, 0), ("five", 65, 1), ("cars", 257, 0)]
# every population of GPU tests 2 and 3, once: what the CPU oracle is asked about
ALL_CASES = list(dict.fromkeys(CASES + [c[:3] for c in TWIN_CASES] + DEAD_FORCE_CASES))
SEEDS = {c: 7100 + 13 * i for i, c in enumerate(ALL_CASES)}


def population(kind, n, rule=0, seed=None):
    """dict(pods, cls, s0 [n, ns], off, dq, script = None | (idx, offsets, rows), box, kind, n, rule):
    two    two TwoD sets, dealt alternately
    sets   riders of the TwoD field over min(n, 256) sets: 33 TwoD riders of 33 sets, 257 riders over the full table of 256
    five   five classes, ten sets, drawn at random (the population of test_random_mixed_population_vs_oracle)
    cars   four cyclists' classes (twod, bicycle, invpend, planarpoint) and every eighth road user a scripted UncontrolledVehicle
    unc    scripted UncontrolledVehicles only: one set, no rider class
    br     two sets, one of them a BalancingRiderBicycle's: keeps the general path
    one    one TwoD set: keeps mid_tick_kernel"""
    seed = SEEDS.get((kind, n, rule), 7000 + n) if seed is None else seed   # (7000 + n: populations of tests that compare bits or counters only)
    box = box_for(n)
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    rng = np.random.default_rng(seed + 1)
    script = None
    if kind == "two":
        base = parameters.default_pod("twod")
        pods, cls = [base, parameters.default_pod("twod", f_0=base.f_0 * 1.6, hfov=2.0)], np.arange(n) % 2
    elif kind == "sets":
        # (one class where one class takes the path - tick.inc: between 257 and 1 023 road users of ONE class keep the general path -,
        # TwoDBicycle and PlanarPointBicycle sets in turn above)
        k = min(n, 256)
        pods, cls = twod_sets(k, ("twod",) if n <= 256 else ("twod", "planarpoint")), np.arange(n) % k
    elif kind == "five":
        pods = five_class_sets()
        cls = rng.integers(0, len(pods), n)
        v = np.minimum(v, 4.8)
    elif kind == "cars":
        pods = [parameters.default_pod(m) for m in ("twod", "bicycle", "invpend", "planarpoint")] + [parameters.default_pod("uncontrolled", hfov=2.5, f_0=9.0)]
        cls = np.arange(n) % 4
        cars = np.arange(3, n, 8)
        cls[cars] = 4
        v = np.minimum(v, 4.8)
        rows = [car_script(x[j], y[j], psi[j], v[j], rows=128) for j in cars]
        script = (cars, np.arange(len(cars) + 1) * 128, np.concatenate(rows))
    elif kind == "unc":
        pods, cls = [parameters.default_pod("uncontrolled")], np.zeros(n, dtype=int)
        rows = [car_script(x[j], y[j], psi[j], v[j], rows=128) for j in range(n)]
        script = (np.arange(n), np.arange(n + 1) * 128, np.concatenate(rows))
    elif kind == "br":
        pods, cls = [parameters.default_pod("twod"), parameters.default_pod("balancingrider")], (np.arange(n) % 5 == 0).astype(int)
    elif kind == "one":
        pods, cls = [parameters.default_pod("twod")], np.zeros(n, dtype=int)
    else:
        raise KeyError(kind)
    out = []
    for p in pods:
        q = _ffi.Params.from_buffer_copy(bytes(p))
        q.priority_rule = rule
        out.append(q)
    ns = max(_ffi.N_STATES[p.model] for p in out)
    return dict(pods=out, cls=np.asarray(cls, dtype=np.int32), s0=wide(x, y, psi, v, ns), off=off, dq=dq, script=script, box=box, kind=kind, n=n, rule=rule)


def road_of(box, verts):
    """two straight edges along the box, `verts` vertices in all, integer sigma (what road_kernel sums as a power of rsq)"""
    h = verts // 2
    xs = np.linspace(-0.3 * box, 1.3 * box, h)
    return (np.array([0, h, 2 * h]), np.r_[np.c_[xs, np.full(h, -3.0)], np.c_[xs, np.full(h, box + 3.0)]], np.array([0.15, 0.2]), np.array([2.0, 2.0]))


def build(c, on, capacity=None, road=None, mid_road=False, dead=()):
    """the population on an Engine, csf_mid_classes(on); dead: road users removed again (dead slots in the middle)"""
    from cyclistsocialforce_amd.engine import Engine
    n = c["s0"].shape[0]
    e = Engine(c["pods"][0], capacity or n + 8)
    e.mid_classes(on)
    if mid_road:
        e.mid_road(True)
    e.set_param_classes(c["pods"])                                 # (before the road users: the widest state from here on)
    e.add_agents(c["s0"], VDES)
    e.set_dest_queue(np.arange(n), c["off"], c["dq"], reset=True)
    e.set_agent_class(np.arange(n), c["cls"])
    if c["script"] is not None:
        e.set_script(*c["script"])
    if road is not None:
        e.set_road(*road)
    if len(dead):
        e.step(0)                                                  # (on the device first: a departure then leaves its slot behind, dead)
        e.remove_agents(np.asarray(dead, dtype=np.int32))
    return e


def oracle_population(c):
    """orc.Population of a population (set_classes, set_script), in the layout as wide as the engine's"""
    from oracle import csf_oracle as orc
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in c["pods"]]
    n, ns = c["s0"].shape
    pop = orc.Population(classes[0], c["s0"], VDES, c["off"], c["dq"], ns=ns)
    pop.set_classes(classes, np.asarray(c["cls"], dtype=np.uint8))
    if c["script"] is not None:
        idx, offs, rows = c["script"]
        length = np.zeros(n, dtype=np.int64)
        length[idx] = np.diff(offs)
        full = np.concatenate([[0], np.cumsum(length)])
        pop.set_script(full, rows)                                 # (idx ascending: the rows are already in slot order)
    return pop


def lacking_rows(c):
    """[n, ns] bool: the state rows the class of every road user lacks (they stay exactly 0)"""
    ns = c["s0"].shape[1]
    width = np.array([_ffi.N_STATES[c["pods"][k].model] for k in c["cls"]])
    return np.arange(ns)[None, :] >= width[:, None]


def ulp32(x):
    return float(np.spacing(np.float32(x)))

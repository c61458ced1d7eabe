"""Batches of independent scenes (include/csf.h: csf_batch_join, csf_step_batch; csf_agent.hip: small_batch_kernel): every member
that the one-wave tick takes runs in one launch per vehicle class, one wave per scene.  Bit for bit against twins stepped by
csf_step, against the golden trajectories of the literal reference and against the oracle; members the batched launch does not
take, the packed read-back, wrong calls and the lifetime of a batch."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import csf_oracle as orc
from conftest import shadow_run
from test_gpu_parity import MODELS, amd, make_engine  # noqa: F401  (amd: fixture)
from test_gpu_small import crowd

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

CLASSES = ["twod", "bicycle", "invpend", "planarpoint", "planarbike", "balancingrider"]
HFOVS = [None, 1.0, 2.5, 4.0]


def scene(i):
    """member i of a mixed batch: class, population 1 .. 32, priority rule, field of view, and a road for some"""
    model = CLASSES[i % 6]
    n = 1 + (7 * i + i // 6) % 32
    rule = (i // 3) % 2
    hfov = HFOVS[(i // 2) % 4]
    road = {0: 2.0, 3: 2.5}.get(i % 7)                        # integer sigma: powers of rsq; fractional: the exp2 / log2 form
    box = 14.0 if n <= 8 else (22.0 if n <= 16 else 30.0)
    if model == "balancingrider":
        box *= 2.0
    return model, n, rule, hfov, road, box, 1000 + i


def build(amd, i, capacity=40):
    model, n, rule, hfov, road, box, seed = scene(i)
    x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
    s0 = np.zeros((n, orc.N_STATES[MODELS[model]])); s0[:, 0] = x; s0[:, 1] = y; s0[:, 2] = psi; s0[:, 3] = v
    over = {} if hfov is None else {"hfov": hfov}
    e = make_engine(amd, model, s0, 5.0, off, dq, rule, capacity=capacity, **over)
    if road is not None:
        xs = np.linspace(-20.0, box + 20.0, 400)
        e.set_road(np.array([0, 400, 800]), np.r_[np.c_[xs, np.full(400, -3.0)], np.c_[xs, np.full(400, box + 3.0)]],
                   np.array([0.15, 0.2]), np.array([road, road]))
    return e


def assert_same(a, b, what):
    sa, pa, za, ta = a.state(with_nav=True)
    sb, pb, zb, tb = b.state(with_nav=True)
    assert ta == tb, what
    assert np.array_equal(sa, sb), what
    assert np.array_equal(pa, pb), what
    assert np.array_equal(za, zb), what
    for u, w in zip(a.integrator_state(), b.integrator_state()):
        assert np.array_equal(u, w), what
    for u, w in zip(a.forces(), b.forces()):
        assert np.array_equal(u, w), what
    assert np.array_equal(a.status(), b.status()), what


def mutate(amd, k, engines):
    """the same change on a member and on its twin"""
    for j, e in enumerate(engines):
        i = j // 2
        if (i + k) % 9 == 0 and e.n < 32:                     # an arrival (with its queue)
            ns = e.ns
            s = np.zeros((1, ns)); s[0, :4] = [3.0 + i % 5, 4.0, 0.3, 4.0]
            e.add_agents(s, 5.0)
            e.set_dest_queue(np.array([e.n - 1]), np.array([0, 2]), np.array([[3.0, 4.0, 0.0], [80.0, 30.0, 0.0]]), reset=True)
        elif (i + k) % 9 == 1 and e.n > 2:                     # a departure
            e.remove_agents(np.array([0], dtype=np.int32))
        elif (i + k) % 9 == 2:
            model, _, rule, _, _, _, _ = scene(i)
            e.set_params(amd.pod(model, priority_rule=rule, hfov=1.5 + 0.1 * (k % 20)))
        elif (i + k) % 9 == 3:
            e.set_v_desired(np.arange(e.n, dtype=np.int32), np.full(e.n, 4.0 + 0.25 * (k % 3)))
        elif (i + k) % 9 == 4:
            s = e.state()
            s[:, 3] *= 0.9
            e.push_state(np.arange(e.n, dtype=np.int32), s)
        elif (i + k) % 9 == 5:
            _, _, _, _, _, box, _ = scene(i)
            xs = np.linspace(-10.0, box + 10.0, 200)
            e.set_road(np.array([0, 200]), np.c_[xs, np.full(200, -2.0 - k % 2)], np.array([0.1]), np.array([2.0 + 0.5 * (k % 2)]))


def test_batch_is_bit_identical_to_members_stepped_alone(amd):
    """64 members of all six classes, populations 1 .. 32, both priority rules, four fields of view, roads with integer and
    fractional sigma: 300 ticks in calls of 50 and of 1, with arrivals, departures, parameters, desired speeds, pushed states
    and roads changed between calls - state, integrator state, forces, destinations, navigation state and status as the twins'"""
    K = 64
    batch = [build(amd, i) for i in range(K)]
    twins = [build(amd, i) for i in range(K)]
    amd.Engine.batch_join(batch)
    calls = [50, 50, 1, 1, 1, 50, 1, 1, 50] + [1] * 48 + [47]
    assert sum(calls) == 300
    inter = [x for pair in zip(batch, twins) for x in pair]
    for k, c in enumerate(calls):
        amd.Engine.step_batch(batch, c)
        for t in twins:
            t.step(c)
        if k % 4 == 3:
            mutate(amd, k, inter)
    for i, (a, b) in enumerate(zip(batch, twins)):
        assert_same(a, b, f"member {i} {scene(i)[:5]}")
    bt = [e.batch_ticks() for e in batch]
    assert sum(t > 0 for t in bt) >= K - 8, bt
    assert all(t.batch_ticks() == 0 for t in twins)
    for e in batch:
        assert e.small_ticks() >= e.batch_ticks()


def test_demo_trajectories_golden_replicated_in_one_batch(amd, golden):
    """the reference's demos (four rider classes, the curve scenario with its road) as 260 members of one batch: every copy
    meets the golden trajectories' tolerances, and the copies of a demo are bit-identical to each other"""
    g = golden("trajectories")
    prefixes = [("demo_twod", "twod"), ("demo_planarpoint", "planarpoint"), ("demo_invpend", "invpend"), ("demo_bicycle", "bicycle"),
                ("road_pp", "planarpoint")]
    members, which = [], []
    for c in range(52):
        for j, (prefix, model) in enumerate(prefixes):
            e = make_engine(amd, model, g[f"{prefix}_s0"], g[f"{prefix}_vdes"], g[f"{prefix}_off"], g[f"{prefix}_dq"], 0)
            if f"{prefix}_verts" in g.files:
                e.set_road(g[f"{prefix}_roff"], g[f"{prefix}_verts"], g[f"{prefix}_F0"], g[f"{prefix}_sigma"])
            members.append(e)
            which.append(j)
    assert len(members) >= 256
    amd.Engine.batch_join(members)
    S = {j: g[f"{p}_S"] for j, (p, _) in enumerate(prefixes)}
    steps = max(s.shape[0] for s in S.values())
    for k in range(1, steps):
        amd.Engine.step_batch(members, 10)
        first = {}
        for e, j in zip(members, which):
            if k >= S[j].shape[0]:
                continue
            got = e.state()
            if j in first:
                assert np.array_equal(got, first[j]), (prefixes[j][0], k)
                continue
            first[j] = got
            Sj = S[j]
            extent = max(np.ptp(Sj[..., 0]), np.ptp(Sj[..., 1]), 1.0)
            np.testing.assert_allclose(got[:, :2], Sj[k][:, :2], rtol=0, atol=1e-4 * extent, err_msg=f"{prefixes[j][0]} sample {k}")
            np.testing.assert_allclose(got[:, 3], Sj[k][:, 3], rtol=0, atol=2e-3, err_msg=f"{prefixes[j][0]} speed sample {k}")
    assert all(e.batch_ticks() == 10 * (steps - 1) for e in members)
    assert all((e.status() == 0).all() for e in members)


class _Batched:
    """a member as conftest.shadow_run sees an engine: step() steps the whole batch"""

    def __init__(self, amd, batch, i):
        self._amd, self._batch, self._e = amd, batch, batch[i]

    def step(self, k=1):
        self._amd.Engine.step_batch(self._batch, k)

    def __getattr__(self, name):
        return getattr(self._e, name)


@pytest.mark.parametrize("pick", [(0, 8, 13), (10, 20, 29)])
def test_members_of_a_mixed_batch_vs_oracle(amd, pick):
    """a few members of a 30-member mixed batch: forces every tick for 30 ticks, then trajectories (oracle shadowing)"""
    def oracle(i):
        model, n, rule, hfov, road, box, seed = scene(i)
        x, y, psi, v, off, dq = crowd(n, seed=seed, box=box)
        s0 = np.zeros((n, orc.N_STATES[MODELS[model]])); s0[:, 0] = x; s0[:, 1] = y; s0[:, 2] = psi; s0[:, 3] = v
        over = {} if hfov is None else {"hfov": hfov}
        pop = orc.Population(orc.default_params(model, priority_rule=rule, **over), s0, 5.0, off, dq)
        if road is not None:
            xs = np.linspace(-20.0, box + 20.0, 400)
            pop.set_road(np.array([0, 400, 800]), np.r_[np.c_[xs, np.full(400, -3.0)], np.c_[xs, np.full(400, box + 3.0)]],
                         np.array([0.15, 0.2]), np.array([road, road]))
        return pop

    batch = [build(amd, i) for i in range(30)]
    amd.Engine.batch_join(batch)
    pops = {i: oracle(i) for i in pick}
    for t in range(30):
        amd.Engine.step_batch(batch, 1)
        for i, pop in pops.items():
            pop.step(1)
            fx, fy = batch[i].forces(); ofx, ofy = pop.forces()
            scale = max(np.hypot(ofx, ofy).max(), 1e-3)
            assert max(np.abs(fx - ofx).max(), np.abs(fy - ofy).max()) < 1e-4 * scale, (i, t)
    for i in pick:                                            # (a fresh batch for each: shadow_run counts the member's ticks)
        batch2 = [build(amd, k) for k in range(30)]
        amd.Engine.batch_join(batch2)
        pop = oracle(i)
        worst, _, _, ref = shadow_run(_Batched(amd, batch2, i), pop, 200, 10)
        assert batch2[i].batch_ticks() == 200
        extent = max(np.ptp(ref[:, 0]), np.ptp(ref[:, 1]), 14.0)
        assert worst < 1e-4 * extent, (i, worst)


def test_members_the_batched_launch_does_not_take(amd, monkeypatch):
    """33 road users, two parameter sets, an UncontrolledVehicle, profiling, a road of 3 000 vertices - beside eligible members
    in one batch: each equals its twin, and batch_ticks shows which members were batched"""
    def make(kind):
        if kind == "big":
            x, y, psi, v, off, dq = crowd(33, seed=5, box=30.0)
            return make_engine(amd, "twod", np.c_[x, y, psi, v, np.zeros(33)], 5.0, off, dq)
        x, y, psi, v, off, dq = crowd(6, seed=6)
        if kind == "unc":                                     # (a prescribed trajectory of 100 rows each)
            e = make_engine(amd, "uncontrolled", np.c_[x, y, psi, v], 5.0, off, dq)
            t = np.arange(100) * 0.01
            rows = np.concatenate([np.c_[x[j] + v[j] * t * np.cos(psi[j]), y[j] + v[j] * t * np.sin(psi[j]), np.full(100, psi[j]),
                                         np.full(100, v[j])] for j in range(6)])
            e.set_script(np.arange(6), np.arange(7) * 100, rows)
            return e
        e = make_engine(amd, "twod", np.c_[x, y, psi, v, np.zeros(6)], 5.0, off, dq)
        if kind == "classes":
            e.set_param_classes([amd.pod("twod"), amd.pod("twod", hfov=1.2)], cls=np.array([0, 1, 0, 1, 0, 1], dtype=np.uint8))
        elif kind == "prof":
            e.profile(1)
        elif kind == "road":
            big = np.c_[np.linspace(-5.0, 300.0, 3000), np.full(3000, -6.0)]
            e.set_road(np.array([0, 3000]), big, np.array([0.15]), np.array([2.0]))
        return e

    kinds = ["ok", "big", "ok", "classes", "unc", "prof", "road", "ok"]
    batch = [make(k) for k in kinds]
    twins = [make(k) for k in kinds]
    amd.Engine.batch_join(batch)
    for c in (1, 5, 1, 20):
        amd.Engine.step_batch(batch, c)
        for t in twins:
            t.step(c)
    for k, a, b in zip(kinds, batch, twins):
        assert np.array_equal(a.state(), b.state()), k
        for u, w in zip(a.forces(), b.forces()):
            assert np.array_equal(u, w), k
    assert [e.batch_ticks() for e in batch] == [27 if k == "ok" else 0 for k in kinds]


@pytest.mark.parametrize("forces", [True, False])
def test_step_batch_and_read_back_in_one_call(amd, forces):
    """csf_step_batch_get_tick = csf_step_batch + csf_get_tick of every member, with outputs left out; one member the batched
    launch does not take (40 road users)"""
    ids = list(range(12))
    batch = [build(amd, i, capacity=48) for i in ids]
    twins = [build(amd, i, capacity=48) for i in ids]
    x, y, psi, v, off, dq = crowd(40, seed=9, box=35.0)
    batch.append(make_engine(amd, "twod", np.c_[x, y, psi, v, np.zeros(40)], 5.0, off, dq))
    twins.append(make_engine(amd, "twod", np.c_[x, y, psi, v, np.zeros(40)], 5.0, off, dq))
    amd.Engine.batch_join(batch)
    for k in (1, 1, 7, 1, 30):
        outs = []
        for j, e in enumerate(batch):
            n = e.n
            o = [np.zeros((n, e.ns)), np.zeros(n, dtype=np.int32), np.zeros((n, 3), dtype=np.uint8),
                 np.zeros(n) if forces else None, np.zeros(n) if forces else None]
            if j % 3 == 1:
                o[1] = None                                   # (any output may be left out)
            outs.append(o)
        ticks = amd.Engine.step_batch_into(batch, k, outs)
        for j, (t, o) in enumerate(zip(twins, outs)):
            t.step(k)
            s, p, z, fx, fy, tk = t.tick_snapshot()
            assert ticks[j] == tk
            assert np.array_equal(o[0], s)
            if o[1] is not None:
                assert np.array_equal(o[1], p)
            assert np.array_equal(o[2].astype(bool), z)
            if forces:
                assert np.array_equal(o[3], fx) and np.array_equal(o[4], fy)
    bt = [e.batch_ticks() for e in batch]
    assert set(bt) <= {0, 40} and bt.count(40) >= len(ids) - 2 and bt[-1] == 0, bt      # (member 3's road is too long for the wave)


def test_wrong_calls_and_lifetime_in_a_fresh_process():
    """refused calls (NULL, count <= 0, a duplicate, a non-member, the wrong order, an engine already in a batch, a loopback
    member), a destroyed member, and 100 join / step / leave / destroy rounds without losing device memory: in a child process"""
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, os.path.join(here, "batch_abi_child.py")], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "PYTHONPATH": os.path.dirname(here)})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "batch abi ok" in r.stdout


def _junctions(seed_shift):
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import Bicycle, InvPendulumBicycle, PlanarPointBicycle, TwoDBicycle

    out = []
    kinds = [TwoDBicycle, Bicycle, PlanarPointBicycle, InvPendulumBicycle, TwoDBicycle, PlanarPointBicycle, Bicycle]
    for j in range(8):
        if j == 5:
            out.append(SocialForceIntersection([], id=f"j{j}"))         # an empty junction
            continue
        cls = kinds[j % len(kinds)]
        dx, dy = 0.7 * j - 2.0, -0.5 * (j % 3)                          # demoCSFstandalone.py:101-118, from varied starts
        a = cls((-6 + dx, dy, 0.05 * j, 5, 0, 0, 0, 0), id="a", saveForces=True)
        a.params.v_desired_default = 4.5
        b = cls((15 + dx, -20 + dy, np.pi / 2, 5, 0, 0, 0, 0), id="b", saveForces=True)
        b.params.v_desired_default = 5.0
        c = cls((13 + dx, -20 - dy, np.pi / 2, 5, 0, 0, 0, 0), id="c", saveForces=True)
        c.params.v_desired_default = 5.0
        a.setDestinations((35, 64, 65), (0, 0, 0))
        b.setDestinations((15, 15, 15), (20, 49, 50))
        c.setDestinations((13, 13, 13), (20, 49, 50))
        out.append(SocialForceIntersection([a, b, c], id=f"j{j}"))
    return out


def test_intersections_stepped_together_equal_their_own_steps():
    """eight junctions of the demo's riders (one empty) for 500 ticks through step_together: vehicle.s, traj, F and hist_n_vecs
    exactly as with .step() on each"""
    from cyclistsocialforce_amd import step_together

    together, alone = _junctions(0), _junctions(0)
    step_together(together, 1)
    for _ in range(449):
        step_together(together)
    step_together(together, 50)
    for _ in range(500):
        for ins in alone:
            ins.step()
    for j, (p, q) in enumerate(zip(together, alone)):
        assert p.hist_n_vecs == q.hist_n_vecs and len(p.hist_n_vecs) == 500, j
        for u, w in zip(p.vehicles, q.vehicles):
            assert np.array_equal(u.s, w.s), j
            assert np.array_equal(u.traj, w.traj), j
            assert np.array_equal(np.asarray(u.F), np.asarray(w.F)), j
            assert np.array_equal(u.trajF, w.trajF), j
        if p.vehicles:
            assert p.engine.batch_ticks() == 500 and q.engine.batch_ticks() == 0, j

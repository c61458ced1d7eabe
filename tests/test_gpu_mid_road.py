"""The road term inside the one-launch tick (include/csf.h: csf_mid_road, csf_mid_road_ticks; csf_mid.hip: the ROAD instances of
mid_tick_kernel and mid_batch_kernel).  "Twin" is always the same engine with the switch OFF, stepped by csf_step: a road
launch in front of every one-launch tick, which is what every engine did before there was a switch.  Bit for bit against twins, alone and
as batch members; off by default; above the cap and on a lattice still two launches; launches that do not grow with the members; the
oracle's forces; the wrong calls in a child process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_parity import amd, make_engine  # noqa: F401  (amd: fixture)
from test_gpu_small import crowd
from test_gpu_batch import assert_same, build as build_small
from test_gpu_mid import anchor, start_state
from mid_road_common import ON_VERTEX, ORACLE_MEMBERS, box_for, member_inputs, oracle_inputs, oracle_member, road

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

CALLS = [50, 1, 1, 50, 1, 37]                                      # (two re-binnings)


def member(amd, model, n, rule, kind, seed, switch=True, spare=8):
    s0, off, dq = member_inputs(model, n, rule, seed)
    e = make_engine(amd, model, s0, 5.0, off, dq, rule, capacity=n + spare)
    if kind is not None:
        e.set_road(*road(kind, box_for(n)))
    if switch:
        e.mid_road(True)
    return e


def same(a, b, what):
    assert_same(a, b, what)
    assert a.near_dropped() == b.near_dropped(), what
    assert a.mid_ticks() == b.mid_ticks(), what


def test_off_by_default(amd):
    """50 TwoD riders beside a 300-vertex edge, alone and as a batch member, nobody touches the switch: the road launch stays, and
    the member stays out of the batched tick"""
    alone = member(amd, "twod", 50, 0, "sigma2", 71, switch=False)
    alone.step(10)
    assert alone.mid_ticks() == 10 and alone.mid_road_ticks() == 0
    batch = [member(amd, "twod", 50, 0, "sigma2", 71, switch=False), member(amd, "twod", 64, 0, None, 72, switch=False),
             member(amd, "twod", 40, 1, None, 73, switch=False)]
    amd.Engine.batch_join(batch)
    amd.Engine.step_batch(batch, 10)
    assert batch[0].mid_road_ticks() == 0 and batch[0].batch_mid_ticks() == 0 and batch[0].mid_ticks() == 10
    assert batch[1].batch_mid_ticks() == 10 and batch[2].batch_mid_ticks() == 10
    same(batch[0], alone, "the batch member and the engine stepped alone")


# (class, road users, priority rule, road, what happens between the calls): one per way the road item can go wrong - the five classes
# at n = 33 (groups of 4: the last group holds one live slot), 40 / 257 / 600 for the two fields' classes, both rules, every NP, a last
# half-empty pass, two tiles, the cap, r = 0, dead slots inside a group
CASES = [("twod", 33, 0, "sigma2", None), ("bicycle", 33, 1, "two", None), ("invpend", 33, 0, "sigma2.5", None),
         ("planarpoint", 33, 1, "mixed", None), ("planarbike", 33, 0, "tiles", None),
         ("twod", 40, 1, "cap", None), ("twod", 257, 0, "two", None), ("twod", 600, 1, "tiles", None),
         ("bicycle", 40, 0, "sigma2", None), ("bicycle", 257, 1, "mixed", None), ("bicycle", 600, 0, "cap", None),
         ("twod", 100, 0, "sigma2", "vertex"), ("bicycle", 48, 1, "two", "vertex"),
         ("twod", 70, 1, "two", "leave"), ("bicycle", 150, 0, "sigma2.5", "leave"), ("invpend", 200, 1, "tiles", "leave")]


@pytest.mark.parametrize("k", range(len(CASES)))
def test_single_scene_is_bit_identical_to_its_twin(amd, monkeypatch, k):
    """state, navigation, integrator state, forces, status, near_dropped and mid_ticks as the twin's after every call of 50, 1, 1, 50, 1,
    37 ticks, and every tick's road term summed inside the one launch; a third of the cases with CSF_DEBUG_POISON=1"""
    model, n, rule, kind, between = CASES[k]
    if k % 3 == 0:
        monkeypatch.setenv("CSF_DEBUG_POISON", "1")
    e, t = member(amd, model, n, rule, kind, 6000 + k), member(amd, model, n, rule, kind, 6000 + k, switch=False)
    done = 0
    for c, ticks in enumerate(CALLS):
        e.step(ticks)
        t.step(ticks)
        done += ticks
        same(e, t, (CASES[k], c))
        fx, fy = e.forces()
        assert np.isfinite(fx).all() and np.isfinite(fy).all(), (CASES[k], c)
        assert e.mid_ticks() == done and e.mid_road_ticks() == done and t.mid_road_ticks() == 0, (CASES[k], c)
        if between == "vertex" and c in (0, 3):                    # a rider exactly on a vertex: the pair it forms has r = 0
            for x in (e, t):
                s = x.state()
                s[3 + c, 0], s[3 + c, 1] = ON_VERTEX
                x.push_state(np.array([3 + c], dtype=np.int32), s[3 + c: 4 + c])
        if between == "leave" and c in (0, 3):                     # departures: dead slots inside a group
            for x in (e, t):
                x.remove_agents(np.array([1, 6 + c, n // 2], dtype=np.int32))


@pytest.mark.parametrize("how", ["above", "lattice"])
def test_above_the_cap_or_on_a_lattice_still_two_launches(amd, monkeypatch, how):
    """2 049 vertices (2 112 padded), or CSF_ROAD_GRID=1: the switch is on and the road launch stays - equal to the twin"""
    if how == "lattice":
        monkeypatch.setenv("CSF_ROAD_GRID", "1")
    kind = "above" if how == "above" else "two"
    e, t = member(amd, "twod", 50, 0, kind, 81), member(amd, "twod", 50, 0, kind, 81, switch=False)
    for ticks in (40, 1, 30):
        e.step(ticks)
        t.step(ticks)
        same(e, t, how)
    assert e.mid_ticks() == 71 and e.mid_road_ticks() == 0


ROAD_MEMBERS = [("twod", 33, 0, "sigma2"), ("twod", 257, 1, "two"), ("twod", 100, 0, "cap"), ("bicycle", 40, 1, "mixed"),
                ("bicycle", 300, 0, "tiles"), ("invpend", 64, 1, "sigma2.5"), ("planarpoint", 90, 0, "two"), ("planarbike", 70, 1, "sigma2")]


def test_road_members_of_a_batch_are_bit_identical_to_twins(amd):
    """eight members with roads (the classes, rules and roads above) beside two mid-size members without a road, a one-wave member and
    one whose road is above the cap; between the calls another road on one member, a road removed, a road given, the switch turned off
    on one member - every member equal to its twin after every call, and counted where it ran"""
    def make(switch):
        es = [member(amd, *m, 7000 + j, switch=switch) for j, m in enumerate(ROAD_MEMBERS)]
        es += [member(amd, "twod", 64, 0, None, 7100, switch=switch), member(amd, "bicycle", 120, 1, None, 7101, switch=switch)]
        es += [build_small(amd, 1), member(amd, "twod", 50, 0, "above", 7102, switch=switch)]
        return es

    batch, twins = make(True), make(False)
    R, PLAIN, SMALL, CAPPED = range(8), (8, 9), 10, 11
    amd.Engine.batch_join(batch)
    done = 0
    road_ticks = [0] * len(batch)
    in_batch = [j in R or j in PLAIN for j in range(len(batch))]
    has_fused_road = [j in R for j in range(len(batch))]
    for c, ticks in enumerate(CALLS):
        amd.Engine.step_batch(batch, ticks)
        for t in twins:
            t.step(ticks)
        done += ticks
        for j, (a, b) in enumerate(zip(batch, twins)):
            same(a, b, (c, j))
            if has_fused_road[j]:
                road_ticks[j] += ticks
            assert a.mid_road_ticks() == road_ticks[j] and b.mid_road_ticks() == 0, (c, j)
        if c == 0:
            for x in (batch[1], twins[1]):                          # another road
                x.set_road(*road("mixed", box_for(257)))
            for x in (batch[3], twins[3]):                          # the road removed: the member goes on in the no-road launch
                x.set_road(np.array([0]), np.zeros((0, 2)), np.zeros(0), np.zeros(0))
            has_fused_road[3] = False
            for x in (batch[8], twins[8]):                          # a road given to a member that had none
                x.set_road(*road("sigma2", box_for(64)))
            has_fused_road[8] = True
            before3, before8 = batch[3].batch_mid_ticks(), batch[8].batch_mid_ticks()
        if c == 2:
            batch[5].mid_road(False)                                # it leaves the batched launch and stays equal to its twin
            has_fused_road[5] = False
            before5 = batch[5].batch_mid_ticks()
    assert batch[3].batch_mid_ticks() == before3 + done - CALLS[0] and batch[8].batch_mid_ticks() == before8 + done - CALLS[0]
    assert batch[5].batch_mid_ticks() == before5 == sum(CALLS[:3]) and batch[5].mid_ticks() == done
    for j, (a, b) in enumerate(zip(batch, twins)):
        assert b.batch_mid_ticks() == 0, j
        if j in R and j != 5:
            assert a.batch_mid_ticks() == done and a.mid_ticks() == done, j
        if j in PLAIN:
            assert a.batch_mid_ticks() == done, j
    assert batch[SMALL].batch_ticks() == done and batch[SMALL].batch_mid_ticks() == 0
    assert batch[CAPPED].batch_mid_ticks() == 0 and batch[CAPPED].mid_road_ticks() == 0 and batch[CAPPED].mid_ticks() == done
    assert all(in_batch[j] or batch[j].batch_mid_ticks() == 0 for j in range(len(batch)))


def test_launches_do_not_scale_with_the_number_of_road_members(amd):
    """8 and 32 road members of one class and rule, 192 ticks in one call: the same number of launches and copies"""
    counts = []
    for K in (8, 32):
        es = [member(amd, "twod", 64, 0, "sigma2", 500 + j) for j in range(K)]
        amd.Engine.batch_join(es)
        amd.Engine.step_batch(es, 192, sync=True)
        assert all(e.batch_mid_ticks() == 192 and e.mid_road_ticks() == 192 for e in es)
        counts.append(es[0].batch_launches())
        assert all(e.batch_launches() == counts[-1] for e in es)
        for e in es:
            e.close()
    print("launches and copies for 192 ticks, 8 and 32 road members:", counts)
    assert counts[0] == counts[1] and 192 <= counts[0] <= 192 + 40, counts


def test_road_members_of_a_batch_vs_oracle(amd):
    """four batched members between two edges against the oracle: the forces of every receiver on every tick for 20 ticks, 1e-4 of the
    largest force, the oracle re-anchored above 300 road users (the bar of test_gpu_batch_mid.py::test_mid_members_of_a_batch_vs_oracle)"""
    es, pops = [], []
    for m in ORACLE_MEMBERS:
        s0, off, dq, over, rd = oracle_inputs(m)
        e = make_engine(amd, m[0], s0, 5.0, off, dq, m[2], **over)
        e.set_road(*rd)
        e.mid_road(True)
        es.append(e)
        pops.append(oracle_member(m))
    amd.Engine.batch_join(es)
    for t in range(20):
        for e, pop, m in zip(es, pops, ORACLE_MEMBERS):
            if m[1] > 300 and t > 0:
                anchor(e, pop)
        amd.Engine.step_batch(es, 1)
        for e, pop, m in zip(es, pops, ORACLE_MEMBERS):
            pop.step(1)
            fx, fy = e.forces(); ofx, ofy = pop.forces()
            assert np.isfinite(ofx).all() and np.isfinite(ofy).all(), (t, m)
            scale = max(np.hypot(ofx, ofy).max(), 1e-3)
            err = max(np.abs(fx - ofx).max(), np.abs(fy - ofy).max())
            print(f"tick {t} {m[0]} {m[1]}: max force deviation {err / scale:.2e} of the largest force")
            assert err < 1e-4 * scale, (t, m)
    assert all(e.batch_mid_ticks() == 20 and e.mid_road_ticks() == 20 for e in es)


def test_wrong_calls_in_a_fresh_process():
    """on = 2, a NULL handle, a call while a calibration data set is held: each refused with nothing changed; CSF_MID_ROAD=1 at creation"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in ("CSF_PAIR_VARIANT", "CSF_MID_ROAD", "CSF_FUSED_MID")}
    r = subprocess.run([sys.executable, os.path.join(here, "mid_road_abi_child.py")], capture_output=True, text=True, timeout=600,
                       env={**env, "PYTHONPATH": os.path.dirname(here)})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mid road abi ok" in r.stdout

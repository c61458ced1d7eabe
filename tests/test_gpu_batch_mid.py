"""Mid-size members of a batch (include/csf.h: csf_step_batch, csf_batch_mid_ticks, csf_batch_launches; csf_mid.hip:
mid_batch_kernel): the members that the one-launch tick takes - 33 ... 2 175 road users of one parameter set, no road - run
tick by tick in one launch per vehicle class and priority rule.  Bit for bit against twins stepped by csf_step, against the
oracle at the bars of test_gpu_mid.py, with planted undecidable pairs, with a recording, across changes of membership, with
poisoned slack, and the number of launches does not grow with the number of members."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import csf_oracle as orc
from conftest import shadow_run
from test_gpu_parity import amd, make_engine  # noqa: F401  (amd: fixture)
from test_gpu_small import crowd
from test_gpu_batch import assert_same, build as build_small
from test_gpu_mid import anchor, start_state

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

# (class, road users, priority rule, field of view): five classes, 33 ... 600 road users, both rules, three fields of view
MEMBERS = [("twod", 33, 0, None), ("twod", 40, 1, 2.0), ("twod", 100, 0, 4.0), ("twod", 257, 1, None), ("twod", 600, 0, 2.0),
           ("bicycle", 33, 1, None), ("bicycle", 48, 0, 4.0), ("bicycle", 150, 1, 2.0), ("bicycle", 300, 0, None), ("bicycle", 450, 1, 4.0),
           ("invpend", 34, 0, None), ("invpend", 64, 1, 2.0), ("invpend", 200, 0, 4.0), ("invpend", 330, 1, None),
           ("planarpoint", 36, 1, None), ("planarpoint", 90, 0, 2.0), ("planarpoint", 260, 1, 4.0), ("planarpoint", 500, 0, None),
           ("planarpoint", 128, 0, None),
           ("planarbike", 35, 0, None), ("planarbike", 70, 1, 4.0), ("planarbike", 190, 0, 2.0), ("planarbike", 320, 1, None),
           ("planarbike", 64, 0, None)]


def box_for(n):
    return max(30.0, 3.2 * np.sqrt(n))


def mid_member(amd, i, spare=8):
    model, n, rule, hfov = MEMBERS[i]
    x, y, psi, v, off, dq = crowd(n, seed=4000 + i, box=box_for(n))
    over = {} if hfov is None else {"hfov": hfov}
    return make_engine(amd, model, start_state(model, x, y, psi, v), 5.0, off, dq, rule, capacity=n + spare, **over)


def other_member(amd, kind):
    """members the batched one-launch tick does not take: one-wave members, and mid-size ones that stay in turn"""
    if kind.startswith("small"):
        return build_small(amd, int(kind[5:]))
    if kind == "road":
        x, y, psi, v, off, dq = crowd(50, seed=71, box=30.0)
        e = make_engine(amd, "twod", start_state("twod", x, y, psi, v), 5.0, off, dq)
        xs = np.linspace(-10.0, 40.0, 300)
        e.set_road(np.array([0, 300]), np.c_[xs, np.full(300, -3.0)], np.array([0.15]), np.array([2.0]))
        return e
    if kind == "classes":
        x, y, psi, v, off, dq = crowd(40, seed=72, box=30.0)
        e = make_engine(amd, "twod", start_state("twod", x, y, psi, v), 5.0, off, dq)
        e.set_param_classes([amd.pod("twod"), amd.pod("twod", hfov=1.2)], cls=(np.arange(40) % 2).astype(np.uint8))
        return e
    if kind == "balancing":
        x, y, psi, v, off, dq = crowd(40, seed=73, box=60.0)
        return make_engine(amd, "balancingrider", start_state("balancingrider", x, y, psi, v), 5.0, off, dq)
    assert kind == "unc"
    x, y, psi, v, off, dq = crowd(6, seed=74)
    e = make_engine(amd, "uncontrolled", np.c_[x, y, psi, v], 5.0, off, dq)
    t = np.arange(100) * 0.01
    rows = np.concatenate([np.c_[x[j] + v[j] * t * np.cos(psi[j]), y[j] + v[j] * t * np.sin(psi[j]), np.full(100, psi[j]),
                                 np.full(100, v[j])] for j in range(6)])
    e.set_script(np.arange(6), np.arange(7) * 100, rows)
    return e


OTHERS = ["small1", "small2", "small4", "road", "classes", "balancing", "unc"]


def change(amd, k, i, e):
    """change k of mid-size member i - the same on the member and on its twin"""
    model, n, rule, hfov = MEMBERS[i]
    what = (i + k) % 5
    if what == 0 and e.n < n + 6:                              # two arrivals, with their queues
        s = np.zeros((2, e.ns)); s[:, :4] = [[1.0 + i % 7, 2.0, 0.3, 4.0], [4.0, 1.0 + i % 5, 1.2, 3.5]]
        e.add_agents(s, 5.0)
        e.set_dest_queue(np.array([e.n - 2, e.n - 1]), np.array([0, 2, 4]),
                         np.array([[s[0, 0], s[0, 1], 0.0], [80.0, 30.0, 0.0], [s[1, 0], s[1, 1], 0.0], [20.0, 90.0, 0.0]]), reset=True)
    elif what == 1:                                            # departures: dead slots
        e.remove_agents(np.array([0, 5 + k], dtype=np.int32))
    elif what == 2:
        e.set_params(amd.pod(model, priority_rule=rule, hfov=1.5 + 0.1 * ((i + k) % 20)))
    elif what == 3:
        e.set_v_desired(np.arange(e.n, dtype=np.int32), np.full(e.n, 4.0 + 0.25 * (k % 3)))
    else:
        s = e.state()
        s[:, 3] *= 0.9
        e.push_state(np.arange(e.n, dtype=np.int32), s)


def same(a, b, what):
    assert_same(a, b, what)
    assert a.near_dropped() == b.near_dropped(), what
    assert a.mid_ticks() == b.mid_ticks(), what


def run_against_twins(amd, ids, others):
    batch = [mid_member(amd, i) for i in ids] + [other_member(amd, k) for k in others]
    twins = [mid_member(amd, i) for i in ids] + [other_member(amd, k) for k in others]
    amd.Engine.batch_join(batch)
    calls = [50, 1, 1, 50, 1, 37]
    assert sum(calls) >= 140
    for k, c in enumerate(calls):
        amd.Engine.step_batch(batch, c)
        for t in twins:
            t.step(c)
        for j, (a, b) in enumerate(zip(batch, twins)):         # (after every call: a later change could paint a difference over)
            same(a, b, f"call {k}, member {j} {MEMBERS[ids[j]] if j < len(ids) else others[j - len(ids)]}")
        if k in (0, 2, 3):
            for j, i in enumerate(ids):
                change(amd, k, i, batch[j])
                change(amd, k, i, twins[j])
    for j, (a, b) in enumerate(zip(batch, twins)):
        what = f"member {j} {MEMBERS[ids[j]] if j < len(ids) else others[j - len(ids)]}"
        same(a, b, what)
        assert b.batch_mid_ticks() == 0 and b.batch_ticks() == 0, what
        if j < len(ids):
            assert a.batch_mid_ticks() > 0 and a.batch_ticks() == 0, what
            assert a.mid_ticks() >= a.batch_mid_ticks(), what
        else:
            assert a.batch_mid_ticks() == 0, what
            assert a.batch_ticks() == (sum(calls) if others[j - len(ids)].startswith("small") else 0), what
    assert batch[0].batch_launches() > 0


def test_mid_members_are_bit_identical_to_twins_stepped_alone(amd):
    """24 mid-size members of five classes, 33 ... 600 road users, both priority rules, three fields of view, beside three
    one-wave members and four that stay in turn (a road, two parameter sets, 40 BalancingRiders, an UncontrolledVehicle): 140
    ticks in calls of 50 and 1 across two re-binnings, with arrivals, departures, parameters, desired speeds and pushed states
    changed between calls - state, navigation, integrator state, forces, status, near_dropped and mid_ticks as the twins'"""
    run_against_twins(amd, list(range(len(MEMBERS))), OTHERS)


def test_poisoned_slack(amd, monkeypatch):
    """a third of the members above with CSF_DEBUG_POISON=1 (0xFF bytes behind every array): still bit-identical"""
    monkeypatch.setenv("CSF_DEBUG_POISON", "1")
    run_against_twins(amd, list(range(0, len(MEMBERS), 3)), ["small1", "road", "unc"])


ORACLE_MEMBERS = [("twod", 100, 1, None, 40.0), ("invpend", 64, 0, None, 40.0), ("bicycle", 300, 1, 4.0, 60.0), ("planarpoint", 500, 1, 2.0, 70.0)]


def oracle_batch(amd):
    es, pops = [], []
    for model, n, rule, hfov, box in ORACLE_MEMBERS:
        x, y, psi, v, off, dq = crowd(n, seed=7 * n + rule, box=box)
        s0 = start_state(model, x, y, psi, v)
        over = {} if hfov is None else {"hfov": hfov}
        es.append(make_engine(amd, model, s0, 5.0, off, dq, rule, **over))
        pops.append(orc.Population(orc.default_params(model, priority_rule=rule, **over), s0, 5.0, off, dq))
    amd.Engine.batch_join(es)
    return es, pops


class _Driven:
    """one member of a batch as shadow_run sees an engine: step() steps the WHOLE batch, so the other members move along"""

    def __init__(self, amd, batch, j):
        self.amd, self.batch, self.e = amd, batch, batch[j]

    def step(self, k):
        self.amd.Engine.step_batch(self.batch, k)

    def __getattr__(self, name):
        return getattr(self.e, name)


def test_mid_members_of_a_batch_vs_oracle(amd):
    """four members of one batch against the oracle at the bars of test_mid_crowds_vs_oracle: forces of every receiver on every
    tick for 20 ticks (1e-4 of the largest force; the oracle re-anchored above 300 road users), trajectories in shadow windows of
    10 over 140 ticks (1e-4 of the extent), destination pointers and navigation states equal.  The batch is driven as a whole:
    every step of the member under comparison is a csf_step_batch of all four."""
    es, pops = oracle_batch(amd)
    for t in range(20):
        for e, pop, m in zip(es, pops, ORACLE_MEMBERS):
            if m[1] > 300 and t > 0:
                anchor(e, pop)
        amd.Engine.step_batch(es, 1)
        for e, pop, m in zip(es, pops, ORACLE_MEMBERS):
            pop.step(1)
            fx, fy = e.forces(); ofx, ofy = pop.forces()
            scale = max(np.hypot(ofx, ofy).max(), 1e-3)
            assert max(np.abs(fx - ofx).max(), np.abs(fy - ofy).max()) < 1e-4 * scale, (t, m)
    assert all(e.batch_mid_ticks() == 20 and e.mid_ticks() == 20 for e in es)
    for j, m in enumerate(ORACLE_MEMBERS):
        es2, pops2 = oracle_batch(amd)
        worst, _, got, ref = shadow_run(_Driven(amd, es2, j), pops2[j], 140, 10)
        e2, n = es2[j], m[1]
        assert e2.batch_mid_ticks() == 140 and (e2.status() == 0).all() and e2.near_dropped() == 0, m
        extent = max(np.ptp(ref[:, 0]), np.ptp(ref[:, 1]), 14.0)
        assert worst < 1e-4 * extent, m
        _, ptr, zn, _ = e2.state(with_nav=True)
        optr, ozn, _, _ = pops2[j].nav()
        np.testing.assert_array_equal(ptr, optr)
        np.testing.assert_array_equal(np.asarray(zn).reshape(n, 3).astype(bool), ozn)


def planted(seed):
    """the construction of test_undecidable_pairs_on_the_one_launch_path: receivers within rounding of a field-of-view edge and of
    the line ahead of a source"""
    rng = np.random.default_rng(seed)
    n = 320
    x, y = rng.uniform(0, 60, n), rng.uniform(0, 60, n)
    psi, v = rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 6, n)
    hf = 2 * np.pi / 3
    for k in range(0, 160, 2):
        r, sgn = rng.uniform(3, 20), (-1) ** k
        if k % 4 == 0:
            ang = psi[k + 1] + sgn * (hf / 2 + rng.choice([-1, 1]) * 10 ** rng.uniform(-9, -7))
            x[k], y[k] = x[k + 1] + r * np.cos(ang), y[k + 1] + r * np.sin(ang)
        else:
            off_ = rng.choice([-1, 1]) * 10 ** rng.uniform(-9, -7)
            x[k + 1] = x[k] + r * np.cos(psi[k]) - off_ * np.sin(psi[k])
            y[k + 1] = y[k] + r * np.sin(psi[k]) + off_ * np.cos(psi[k])
            psi[k + 1] = psi[k] + np.pi + rng.uniform(-0.3, 0.3)
    reach = np.array([8.0, 25.0, 60.0, 61.0])
    dq = np.zeros((n, 5, 3)); dq[:, 0, 0], dq[:, 0, 1] = x, y
    dq[:, 1:, 0] = x[:, None] + reach[None, :] * np.cos(psi)[:, None]
    dq[:, 1:, 1] = y[:, None] + reach[None, :] * np.sin(psi)[:, None]
    return start_state("twod", x, y, psi, v), np.arange(n + 1) * 5, dq.reshape(-1, 3)


def test_undecidable_pairs_in_members_of_a_batch(amd):
    """the planted pairs in two members of a batch: forces 1e-4 against the oracle on every tick, bit-identical to twins that
    are stepped alone and have their states anchored the same way, nothing dropped"""
    seeds = (3, 11)
    batch = [make_engine(amd, "twod", *((lambda s0, off, dq: (s0, 5.0, off, dq))(*planted(s)))) for s in seeds]
    twins = [make_engine(amd, "twod", *((lambda s0, off, dq: (s0, 5.0, off, dq))(*planted(s)))) for s in seeds]
    pops = [(lambda s0, off, dq: orc.Population(orc.default_params("twod"), s0, 5.0, off, dq))(*planted(s)) for s in seeds]
    amd.Engine.batch_join(batch)
    for t in range(12):
        amd.Engine.step_batch(batch, 1)
        for e, tw, pop in zip(batch, twins, pops):
            tw.step(1); pop.step(1)
            fx, fy = e.forces(); ofx, ofy = pop.forces()
            scale = max(np.hypot(ofx, ofy).max(), 1e-3)
            assert max(np.abs(fx - ofx).max(), np.abs(fy - ofy).max()) < 1e-4 * scale, t
            same(e, tw, t)
            anchor(e, pop)                                     # (the planted geometry is rounding-sensitive by construction)
    assert all(e.batch_mid_ticks() == 12 and e.near_dropped() == 0 for e in batch)


def test_recording_mid_members(amd):
    """csf_record with forces on mid-size members: 130 ticks in calls of 50 / 1 / 79, batch_recorded equals the twins' recorded"""
    ids = [0, 2, 6, 11, 15, 20]
    batch, twins = [mid_member(amd, i) for i in ids], [mid_member(amd, i) for i in ids]
    for e in batch + twins:
        e.record(1, 200, True)
    amd.Engine.batch_join(batch)
    for c in (50, 1, 79):
        amd.Engine.step_batch(batch, c)
        for t in twins:
            t.step(c)
    got = amd.Engine.batch_recorded(batch, 130)
    for j, (g, t) in enumerate(zip(got, twins)):
        S, F = t.recorded(0, 130)
        assert g[2] == 0 and np.array_equal(g[0], S) and np.array_equal(g[1], F), MEMBERS[ids[j]]
        assert batch[j].batch_mid_ticks() == 130
        same(batch[j], t, j)


def grow(e, k):
    s = np.zeros((k, e.ns)); s[:, 0] = 2.0 + np.arange(k); s[:, 1] = 1.0; s[:, 2] = 0.4; s[:, 3] = 4.0
    e.add_agents(s, 5.0)
    q = np.zeros((k, 2, 3)); q[:, 0, :2] = s[:, :2]; q[:, 1, 0] = s[:, 0] + 60.0; q[:, 1, 1] = 40.0
    e.set_dest_queue(np.arange(e.n - k, e.n), np.arange(k + 1) * 2, q.reshape(-1, 3), reset=True)


def test_membership_moves(amd, monkeypatch):
    """a member that grows from 30 to 36 road users between calls and shrinks again; a batch whose mid-size members drop to one
    (the other gets a road), which is then stepped in turn; CSF_MID_BELOW=200 on a member of 300; CSF_BATCH_MID=0 - all equal
    to twins"""
    def thirty():
        x, y, psi, v, off, dq = crowd(30, seed=90, box=25.0)
        return make_engine(amd, "twod", start_state("twod", x, y, psi, v), 5.0, off, dq, capacity=48)

    def both(f):
        return f(), f()

    g, tg = both(thirty)
    for e in (g, tg):
        e.record(1, 200, True)                                  # (its tick word in device memory changes hands with the path)
    a, ta = both(lambda: mid_member(amd, 2))
    b, tb = both(lambda: mid_member(amd, 11))
    monkeypatch.setenv("CSF_MID_BELOW", "200")
    c, tc = both(lambda: mid_member(amd, 8))                   # (300 road users: above its CSF_MID_BELOW)
    monkeypatch.delenv("CSF_MID_BELOW")
    batch, twins = [g, a, b, c], [tg, ta, tb, tc]
    amd.Engine.batch_join(batch)

    def go(k):
        amd.Engine.step_batch(batch, k)
        for t in twins:
            t.step(k)
        for j, (p, q) in enumerate(zip(batch, twins)):
            same(p, q, j)

    go(10)
    assert g.batch_ticks() == 10 and g.batch_mid_ticks() == 0 and a.batch_mid_ticks() == 10 and b.batch_mid_ticks() == 10
    assert c.batch_mid_ticks() == 0 and c.mid_ticks() == 0
    grow(g, 6); grow(tg, 6)
    go(70)                                                      # (across a re-binning)
    assert g.batch_ticks() == 10 and g.batch_mid_ticks() == 70
    # ... and back: through the host mirror the departures close their holes (30 slots, 30 road users: one wave again)
    for e in (g, tg):
        e.set_incremental(False)
        e.remove_agents(np.arange(30, 36, dtype=np.int32))
        e.set_incremental(True)
    go(10)
    assert g.batch_ticks() == 20 and g.batch_mid_ticks() == 70
    go(1)
    assert g.batch_ticks() == 21 and g.batch_mid_ticks() == 70
    S, F, first = amd.Engine.batch_recorded(batch, 11, only=[g])[0]   # (the samples since the 30 are among themselves again)
    tS, tF = tg.recorded(80, 11)
    assert first == 80 and np.array_equal(S, tS) and np.array_equal(F, tF)
    # the mid-size members drop to one: g and b get roads
    for e in (g, tg, b, tb):
        xs = np.linspace(-10.0, 60.0, 200)
        e.set_road(np.array([0, 200]), np.c_[xs, np.full(200, -4.0)], np.array([0.15]), np.array([2.0]))
    before = a.batch_mid_ticks()
    go(20)
    assert a.batch_mid_ticks() == before and a.mid_ticks() == ta.mid_ticks() and b.batch_mid_ticks() == 91
    amd.Engine.batch_leave(batch)
    monkeypatch.setenv("CSF_BATCH_MID", "0")
    batch, twins = [mid_member(amd, i) for i in (1, 6, 12)], [mid_member(amd, i) for i in (1, 6, 12)]
    amd.Engine.batch_join(batch)
    go(70)
    assert all(e.batch_mid_ticks() == 0 and e.mid_ticks() == 70 for e in batch)


def test_a_member_leaves_the_batched_tick_at_a_re_binning_inside_a_call(amd, monkeypatch):
    """3 072 road users with CSF_MID_BELOW=4000: the arrivals between two calls leave the engine's pair kernel as it was chosen
    (the plain one), so the member starts the call in the batched one-launch tick; the re-binning inside the call chooses the
    cull-first kernel for that size (CSF_REBIN_CHURN keeps the arrivals from re-binning at once), the one-launch tick no longer takes the member, and it finishes the call in turn - equal
    to its twin, which does the same alone, after a read-back in front of the call (the host mirror was current)"""
    monkeypatch.setenv("CSF_MID_BELOW", "4000")
    monkeypatch.setenv("CSF_REBIN_CHURN", "1000000000")        # (so many arrivals would re-bin on the call's first ticks)
    n0, n1 = 600, 3072

    def big():
        x, y, psi, v, off, dq = crowd(n0, seed=321, box=90.0)
        return make_engine(amd, "twod", start_state("twod", x, y, psi, v), 5.0, off, dq, capacity=3200)

    def more(e):
        x, y, psi, v, off, dq = crowd(n1 - n0, seed=322, box=180.0)
        e.add_agents(start_state("twod", x + 95.0, y, psi, v), 5.0)
        e.set_dest_queue(np.arange(n0, n1), off, dq + np.array([95.0, 0.0, 0.0]), reset=True)

    m, tm = big(), big()
    monkeypatch.delenv("CSF_MID_BELOW")
    monkeypatch.delenv("CSF_REBIN_CHURN")
    a, ta = mid_member(amd, 2), mid_member(amd, 2)
    b, tb = mid_member(amd, 15), mid_member(amd, 15)
    batch, twins = [m, a, b], [tm, ta, tb]
    amd.Engine.batch_join(batch)
    amd.Engine.step_batch(batch, 40)
    for t in twins:
        t.step(40)
    assert m.batch_mid_ticks() == 40
    more(m); more(tm)
    for p, q in zip(batch, twins):
        same(p, q, "before the call")                           # (a read-back: the host mirror is current)
    amd.Engine.step_batch(batch, 60)                            # (the re-binning of tick 64 is inside)
    for t in twins:
        t.step(60)
    for j, (p, q) in enumerate(zip(batch, twins)):
        same(p, q, j)
    print("batched one-launch ticks of the member that left:", m.batch_mid_ticks(), "of", m.mid_ticks(), "one-launch ticks")
    assert 40 < m.batch_mid_ticks() < 100 and m.mid_ticks() == m.batch_mid_ticks()
    assert a.batch_mid_ticks() == 100 and b.batch_mid_ticks() == 100
    amd.Engine.step_batch(batch, 5)
    for t in twins:
        t.step(5)
    for j, (p, q) in enumerate(zip(batch, twins)):
        same(p, q, j)
    assert a.batch_mid_ticks() == 105


def test_launches_do_not_scale_with_the_number_of_members(amd):
    """8 and 32 members of one class, 64 road users each, 192 ticks in one call (three re-binnings): the same number of launches
    and copies - neither the tick nor the periodic work is per member."""
    counts = []
    for K in (8, 32):
        es = []
        for j in range(K):
            x, y, psi, v, off, dq = crowd(64, seed=500 + j, box=30.0)
            es.append(make_engine(amd, "twod", start_state("twod", x, y, psi, v), 5.0, off, dq))
        amd.Engine.batch_join(es)
        amd.Engine.step_batch(es, 192, sync=True)
        assert all(e.batch_mid_ticks() == 192 for e in es)
        counts.append(es[0].batch_launches())
        assert all(e.batch_launches() == counts[-1] for e in es)
        for e in es:
            e.close()
    print("launches and copies for 192 ticks, 8 and 32 members:", counts)
    assert counts[0] == counts[1] and 192 <= counts[0] <= 192 + 40, counts


def test_wrong_calls_and_lifetime_in_a_fresh_process():
    """NULL arguments, a non-member, and 50 join / step / leave / destroy rounds with mid-size members without losing device
    memory: in a child process"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k != "CSF_PAIR_VARIANT"}
    r = subprocess.run([sys.executable, os.path.join(here, "batch_mid_abi_child.py")], capture_output=True, text=True, timeout=900,
                       env={**env, "PYTHONPATH": os.path.dirname(here)})
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "batch mid abi ok" in r.stdout

"""The order in which a workgroup of pair_cull_kernel hands its receivers to its waves (csf_pair.hip: COMPACT; csf_handout.h):
heaviest visit first by default, index order with CSF_EXPERT=1 CSF_HANDOUT=index.  Which wave takes a receiver, and when, enters
no sum - a receiver's visit to a tile is one wave's, its noted corrections are added by that wave in the order they were noted,
tiles stay separated by barriers - so the two orders must agree to the last bit: forces and their parts (the repulsive part is the
sum of the launch's partial sums), states, navigation and integrator states, status words, and the kernel's own counters as
integers; nothing may be dropped from a wave's list of noted pairs in either order.

Every case steps two engines of one process through the same ticks, one per order (the knobs are read per engine, in csf_create).
"""
import numpy as np
import pytest

import pair_plain_f32_common as pp
from test_gpu_chase import crowd
from test_gpu_parity import amd  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.cull_variant]

KNOBS = ("CSF_SEGMENTS", "CSF_EXPERT", "CSF_RPB", "CSF_WIDE", "CSF_FAR_EPS", "CSF_HANDOUT", "CSF_REBIN_TICKS", "CSF_CHASE")


def make(amd, monkeypatch, env, s0, off, dq, rule=0, sets=None, classes=None, **kw):
    """an engine created under exactly the knobs of `env` (and the cull-first kernel pinned, as the recorded fixtures pin it)"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n = s0.shape[0]
    pods = [amd.pod("twod", priority_rule=rule, **dict(kw, **s)) for s in (sets or [dict()])]
    e = amd.Engine(pods[0], n + 256)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    if sets is not None:
        e.set_param_classes(pods, classes)
    return e


def same(a, b):
    """a, b: engines after the same ticks - equal to the last bit, counters included"""
    sa, pa, za, ta = a.state(with_nav=True)
    sb, pb, zb, tb = b.state(with_nav=True)
    assert ta == tb and np.array_equal(sa.view(np.uint64), sb.view(np.uint64)) and np.array_equal(pa, pb) and np.array_equal(za, zb)
    fa, fb = np.c_[a.forces()], np.c_[b.forces()]
    assert np.array_equal(fa.view(np.uint64), fb.view(np.uint64)), int((fa != fb).any(axis=1).sum())
    qa, qb = np.c_[a.force_parts()], np.c_[b.force_parts()]          # (destination and repulsive part: the latter is the partial sums added up)
    assert np.array_equal(qa.view(np.uint64), qb.view(np.uint64)), int((qa != qb).any(axis=1).sum())
    for x, y in zip(a.integrator_state(), b.integrator_state()):
        assert np.array_equal(x, y)
    assert np.array_equal(a.status(), b.status()) and (a.status() == 0).all()
    assert a.near_dropped() == 0 and b.near_dropped() == 0
    ca, ka = a.count_pairs(detail=True)
    cb, kb = b.count_pairs(detail=True)
    assert ka == kb == "pair_cull_kernel", (ka, kb)
    keys = ("evaluated", "tested", "full_passes", "partial_passes")
    print("counters", [ca[k] for k in keys])
    assert [ca[k] for k in keys] == [cb[k] for k in keys] and ca["evaluated"] > 0


def both_orders(amd, monkeypatch, env, stretches, *args, **kw):
    new = make(amd, monkeypatch, dict(env, CSF_CHASE="0"), *args, **kw)
    old = make(amd, monkeypatch, dict(env, CSF_CHASE="0", CSF_EXPERT="1", CSF_HANDOUT="index"), *args, **kw)
    for t in stretches:
        new.step(t); old.step(t)
        same(new, old)
    new.close(); old.close()


def test_several_tiles_per_workgroup_across_a_rebinning(amd, monkeypatch):
    """(a) 4 096 riders in 100 m: the four-wave workgroup walks several tiles of 1 024 sources; 20 ticks, re-binned every 8"""
    both_orders(amd, monkeypatch, {"CSF_REBIN_TICKS": "8"}, (1, 6, 13), *pp.population("rpb16"))


def test_crowd_with_near_pairs_and_hand_overs(amd, monkeypatch):
    """(b) the crowd of test_gpu_chase.py, 4 096 in 45 m with hfov 4.0: a wave's list of noted pairs is corrected between
    receivers there, so corrections added in another order would show"""
    both_orders(amd, monkeypatch, {}, (1, 9), *crowd(4096, 45.0, 11, 5), hfov=4.0)


def test_priority_to_the_right(amd, monkeypatch):
    """(c) the P2R instantiation"""
    both_orders(amd, monkeypatch, {}, (1, 4), *pp.population("p2r"), rule=1)


def test_two_parameter_sets_in_one_grid(amd, monkeypatch):
    """(d) the SEG instantiation: two sets of 2 048 riders in the class-segmented order"""
    both_orders(amd, monkeypatch, {"CSF_SEGMENTS": "1"}, (1, 4), *pp.population("seg"), sets=pp.SETS, classes=pp.classes("seg"))


def test_sixteen_receivers_per_wide_workgroup(amd, monkeypatch):
    """(e) the wide workgroup with 16 receivers, as tests/pair_plain_f32_common.py reaches it"""
    both_orders(amd, monkeypatch, dict(pp.CASES["rpb16"]["env"]), (1, 4), *pp.population("rpb16"))


def test_side_by_side_ticks_on_the_new_order(amd, monkeypatch):
    """(f) the per-agent launch beside the pair launch (CSF_CHASE=2) against the launches in turn, both heaviest first, 50 ticks of
    the crowd: the hand-overs and the tagged partial sums of that path do not depend on the order either"""
    pop = crowd(4096, 45.0, 11, 5)
    a = make(amd, monkeypatch, {"CSF_CHASE": "0"}, *pop, hfov=4.0)
    b = make(amd, monkeypatch, {"CSF_CHASE": "2"}, *pop, hfov=4.0)
    a.step(50); b.step(50)
    same(a, b)
    assert a.chase_ticks() == 0 and b.chase_ticks() >= 50 - 8, b.chase_ticks()
    a.close(); b.close()

"""Heaviest group first (csrc/csf_wg_order.h): with CSF_WG_ORDER=1 the receiver groups of a source chunk are handed to the pair
kernel's workgroups by an order table formed from the costs an earlier launch left.  The change only moves work between
workgroups - a group's sums go to the slots of its receivers whoever serves it - so everything must equal, to the last bit, what
the same engine computes with CSF_WG_ORDER=0 in a fresh process: states, forces, destination pointers, navigation states and the
four counters of csf_count_pairs after every stretch of ticks, with nothing dropped from a list of noted pairs either way.

Cases (tests/wg_order_common.py): the smallest population that takes the headline instantiation (8 192: 32 receivers per
8-wave workgroup, 256 groups x 4 chunks) over two re-binnings with an order every 4 ticks; 8 200 (ragged last group, live
sentinel tail); 4 096 with priority to the right (16 receivers, two chunks); the crowd of test_gpu_chase.py in one csf_step of
300 ticks, in turn and side by side - the host far ahead of the device, where a table read while it is written would show;
departures, arrivals and pushed states between ticks.  Beside the comparison the in-process side reads the tables back: every
row of an order in use is a permutation, the cost table adds up to 28 x tested + 58 x evaluated of csf_count_pairs on the same
state, and the order is dropped after a change of grid or tiles and comes back.  (CSF_WG_ORDER_MIN=0 in every case: by default grids of
fewer than 2 048 workgroups - all of these - keep index order.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sift_bookkeeping_common as sb
import wg_order_common as woc

pytestmark = [pytest.mark.gpu, pytest.mark.cull_variant]

HERE = os.path.dirname(os.path.abspath(__file__))


def reference(name, tmp_path, monkeypatch):
    """the case with CSF_WG_ORDER=0, in a process of its own"""
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ, CSF_WG_ORDER="0")
    env.pop("CSF_EXPERT", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "wg_order_common.py"), name, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(out)


def ordered(name, monkeypatch, inspect=None, mode="1"):
    monkeypatch.setenv("CSF_WG_ORDER", mode)
    if mode == "index":
        monkeypatch.setenv("CSF_EXPERT", "1")
    return woc.run(name, inspect, monkeypatch.setenv)


def same(a, b):
    assert sorted(a.keys()) == sorted(b.keys())
    for k in sorted(a.keys()):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype, k
        if x.dtype.kind == "f":
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64)), (k, int((x != y).sum()))
        else:
            assert np.array_equal(x, y), k
        if k.endswith("_near_dropped"):
            assert x[0] == 0 and y[0] == 0, k
        if k.endswith("_status"):
            assert (x == 0).all(), k
        if k.endswith("_counters"):
            assert x[0] > 0, k


class Tables:
    """what the in-process side sees of the tables after every stretch"""

    def __init__(self):
        self.seen = []

    def __call__(self, e, k):
        t = e.wg_order_tables()
        assert t is not None
        groups, chunks, used, cost, order = t
        if used:
            assert order.shape == (chunks, groups)
            assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(groups, dtype=np.int32), (chunks, 1)))
        self.seen.append((groups, chunks, used))
        self.chase_ticks = e.chase_ticks()
        return cost


@pytest.mark.parametrize("name", ["headline_8192", "ragged_8200", "p2r_4096"])
def test_equal_to_index_order(name, tmp_path, monkeypatch):
    """(a) - (c): the orders come and go with the re-binnings, the results do not move"""
    tb = Tables()
    got = ordered(name, monkeypatch, tb)
    same(got, reference(name, tmp_path, monkeypatch))
    print(name, tb.seen)
    if name == "headline_8192":
        assert all((g, c) == (256, 4) for g, c, _ in tb.seen), tb.seen      # 32 receivers per workgroup, four source chunks
    assert not tb.seen[0][2] and tb.seen[-1][2], tb.seen          # the first tick has no costs to go by; later ticks have an order


@pytest.mark.parametrize("name", ["crowd_in_turn", "crowd_side_by_side"])
def test_crowd_300_ticks_in_one_step(name, tmp_path, monkeypatch):
    """(d) near pairs, early drains, hand-overs; the host runs 300 ticks ahead of the device"""
    tb = Tables()
    got = ordered(name, monkeypatch, tb)
    same(got, reference(name, tmp_path, monkeypatch))
    assert tb.seen[-1][2], tb.seen
    if name == "crowd_side_by_side":       # (the path is entered within the first ticks: tests/test_gpu_chase.py)
        assert tb.chase_ticks >= 300 - 8, tb.chase_ticks
    else:
        assert tb.chase_ticks == 0


def test_side_by_side_equals_in_turn(monkeypatch):
    ta, tb = Tables(), Tables()
    a = ordered("crowd_in_turn", monkeypatch, ta)
    b = ordered("crowd_side_by_side", monkeypatch, tb)
    same(a, b)
    assert ta.chase_ticks == 0 and tb.chase_ticks >= 300 - 8, (ta.chase_ticks, tb.chase_ticks)


def test_population_changes_and_pushed_states(tmp_path, monkeypatch):
    """(e) after departures and arrivals, and after csf_push_state, the launches fall back to index order and the order comes back"""
    tb = Tables()
    got = ordered("population_changes", monkeypatch, tb)
    same(got, reference("population_changes", tmp_path, monkeypatch))
    print(tb.seen)
    assert all(u for _, _, u in tb.seen), tb.seen                  # (six ticks after every change an order is in use again)


def test_order_dropped_at_once_after_a_change(monkeypatch):
    """(e) the tick right after a change of the population runs in index order"""
    monkeypatch.setenv("CSF_WG_ORDER", "1")
    monkeypatch.setenv("CSF_WG_ORDER_TICKS", "4")
    monkeypatch.setenv("CSF_CHASE", "0")
    monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    monkeypatch.setenv("CSF_WG_ORDER_MIN", "0")
    from cyclistsocialforce_amd import parameters
    from cyclistsocialforce_amd.engine import Engine

    n = 8192
    s0, off, dq = woc.crowd(n, 140.0, 31)
    e = Engine(parameters.default_pod("twod"), n + 512)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    e.step(1)
    assert not e.wg_order_tables()[2]
    e.step(1)
    assert not e.wg_order_tables()[2]
    e.step(1)
    assert e.wg_order_tables()[2]                                   # costs of tick 0 -> order of tick 2
    idx = np.arange(16)
    e.push_state(idx, e.state()[idx])
    e.step(1)
    assert not e.wg_order_tables()[2]
    e.step(3)
    assert e.wg_order_tables()[2]
    e.close()


@pytest.mark.parametrize("mode", ["1", "index"])
def test_costs_add_up_to_the_counters(mode, monkeypatch):
    """(f) csf_count_pairs on a state, then one tick from that state: the tick's cost table sums to 28 x tested + 58 x evaluated"""
    monkeypatch.setenv("CSF_WG_ORDER", mode)
    monkeypatch.setenv("CSF_EXPERT", "1")
    monkeypatch.setenv("CSF_WG_ORDER_TICKS", "2")
    monkeypatch.setenv("CSF_CHASE", "0")
    monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    monkeypatch.setenv("CSF_WG_ORDER_MIN", "0")
    from cyclistsocialforce_amd import parameters
    from cyclistsocialforce_amd.engine import Engine

    n = 8200
    s0, off, dq = woc.crowd(n, 140.0, 32)
    e = Engine(parameters.default_pod("twod"), n + 512)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    for k in range(5):
        c, name = e.count_pairs(detail=True)
        assert name == "pair_cull_kernel"
        e.step(1)
        groups, chunks, used, cost, order = e.wg_order_tables()
        assert groups == (n + 31) // 32 and cost.shape == (chunks, groups)
        assert int(cost.astype(np.int64).sum()) == 28 * c["tested"] + 58 * c["evaluated"], k
        assert used == (mode == "1" and k >= 2)
        if used:
            assert np.array_equal(np.sort(order, axis=1), np.tile(np.arange(groups, dtype=np.int32), (chunks, 1)))
    e.close()


def test_shipped_defaults_on_a_grid_they_act_on(tmp_path, monkeypatch):
    """16 384 riders, 512 groups x 8 chunks, no knob of the order set: CSF_WG_ORDER_MIN, CSF_WG_ORDER_TICKS and CSF_CHASE as shipped"""
    for k in ("CSF_WG_ORDER_MIN", "CSF_WG_ORDER_TICKS", "CSF_CHASE", "CSF_EXPERT"):
        monkeypatch.delenv(k, raising=False)
    tb = Tables()
    got = ordered("defaults_16384", monkeypatch, tb)
    same(got, reference("defaults_16384", tmp_path, monkeypatch))
    assert all((g, c) == (512, 8) for g, c, _ in tb.seen), tb.seen
    assert [u for _, _, u in tb.seen] == [False, True, True], tb.seen


@pytest.mark.parametrize("mode", ["1", "index"])
@pytest.mark.parametrize("case", list(sb.CASES))
def test_recorded_fixtures_with_the_tables_on(case, mode, monkeypatch):
    """(g) the recorded bits of tests/test_gpu_sift_bookkeeping.py (forces, states, counters of three single ticks), with costs and
    orders kept on these small grids (CSF_WG_ORDER_MIN=0) and an order formed at every tick: heaviest first, and in index order"""
    from cyclistsocialforce_amd import parameters
    from cyclistsocialforce_amd.engine import Engine

    sb.set_env(case, monkeypatch.setenv, lambda k: monkeypatch.delenv(k, raising=False))
    monkeypatch.setenv("CSF_WG_ORDER", mode)
    monkeypatch.setenv("CSF_EXPERT", "1")
    monkeypatch.setenv("CSF_WG_ORDER_MIN", "0")
    monkeypatch.setenv("CSF_WG_ORDER_TICKS", "1")
    g = np.load(sb.fixture_path(case))
    s0, off, dq = sb.population(case)
    n = s0.shape[0]
    e = Engine(parameters.default_pod("twod", **sb.overrides(case)), n)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    used = []
    for t in range(sb.TICKS):
        e.step(1)
        s, _, _, fx, fy, _ = e.tick_snapshot(forces=True)
        tabs = e.wg_order_tables()
        assert tabs is not None
        used.append(tabs[2])
        if tabs[2]:
            assert np.array_equal(np.sort(tabs[4], axis=1), np.tile(np.arange(tabs[0], dtype=np.int32), (tabs[1], 1)))
        assert np.array_equal(fx.view(np.uint64), g["fx"][t].view(np.uint64)), (case, t, int((fx != g["fx"][t]).sum()))
        assert np.array_equal(fy.view(np.uint64), g["fy"][t].view(np.uint64)), (case, t, int((fy != g["fy"][t]).sum()))
        assert sb.digest(s) == str(g["state_digests"][t]), (case, t)
        c, kernel = e.count_pairs(detail=True)
        assert kernel == "pair_cull_kernel"
        assert [c["evaluated"], c["tested"], c["full_passes"], c["partial_passes"]] == g["counts"][t].tolist(), (case, t)
    assert np.array_equal(s.view(np.uint64), g["states_last"].view(np.uint64))
    assert e.near_dropped() == 0 and (e.status() == 0).all()
    assert used == [False, False, mode == "1"], used        # (costs of tick 0 -> order of tick 2)
    e.close()

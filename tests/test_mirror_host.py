"""PopulationMirror (no GPU): the bulk arrays of a population and what happens to them - adoption, ring growth, widening,
compaction on removal, the watched shadow - on stub vehicles, at capacity 8 with a ring of 6 columns so that it wraps within a
few ticks."""
import numpy as np
import pytest

from cyclistsocialforce_amd.mirror import PopulationMirror

CAP, T = 8, 6


class _Stub:
    """what the mirror touches of a vehicle"""
    uncontrolled = False
    saveForces = False
    drawing = None

    def __init__(self, k, seed=0, i=0):
        w = self.N_STATES
        rng = np.random.default_rng(1000 * seed + k)
        self._index, self._F = k, []
        self._s = rng.normal(size=w)
        self.traj = rng.normal(size=(w, T))
        self.znav = rng.random(3) < 0.5
        self.i, self.destpointer, self.force = int(i), int(rng.integers(0, 9)), tuple(rng.normal(size=2))

    def update_drawing(self, Fres=None):
        pass


class _Five(_Stub):
    N_STATES = 5


class _Six(_Stub):
    N_STATES = 6


class _Car(_Stub):
    N_STATES = 4
    uncontrolled = True


def _seen(v):
    """everything a vehicle shows of its row, as private copies"""
    return dict(s=v._s.copy(), znav=v.znav.copy(), traj=v.traj.copy(), i=v.i, destpointer=v.destpointer, force=v.force)


def _same(seen, v):
    return (all(np.array_equal(seen[k], getattr(v, "_s" if k == "s" else k)) for k in ("s", "znav", "traj"))
            and (seen["i"], seen["destpointer"], seen["force"]) == (v.i, v.destpointer, v.force))


def _adopt(m, new):
    ns = m.ns
    s0 = np.zeros((len(new), ns))
    for k, v in enumerate(new):
        s0[k, : v._s.size] = v._s
    m.adopt(new, s0, np.arange(len(new), dtype=float), T)


def _row_values(m, v):
    """the vehicle's scalars as the mirror holds them (a bound Vehicle reads them there)"""
    return m.i_of(v), m.pointer_of(v), (float(m.live()[3][v._index]), float(m.live()[4][v._index]))


def _tick(m, rng):
    s, ptr, zn, fx, fy = m.live()
    s[:], fx[:], fy[:] = rng.normal(size=s.shape), rng.normal(size=fx.shape), rng.normal(size=fy.shape)
    m.book_tick(fx, fy, True, 1)


def _mirror(vehicles, ns=5, cap=CAP):
    m = PopulationMirror()
    m.allocate(cap, ns)
    _adopt(m, vehicles)
    return m


def test_compaction_keeps_the_survivors_and_hands_the_leavers_private_copies():
    vs = [_Five(k, i=(2 * k) % T) for k in range(6)]
    m = _mirror(vs)
    rng = np.random.default_rng(3)
    for _ in range(4):
        _tick(m, rng)
    assert len({m.i_of(v) for v in vs}) > 1                          # unequal vehicle.i
    for v in vs:                                                       # (stubs keep plain attributes: what a Vehicle would read)
        v.i, v.destpointer, v.force = _row_values(m, v)
    before = [_seen(v) for v in vs]
    m.compact([1, 2, 4])
    assert m.vehicles == [vs[1], vs[2], vs[4]] and [v._index for v in m.vehicles] == [0, 1, 2]
    S, ptr, zn, fx, fy = m.live()
    for k, v in zip((1, 2, 4), m.vehicles):
        assert np.array_equal(before[k]["s"], v._s) and np.array_equal(before[k]["znav"], v.znav) and np.array_equal(before[k]["traj"], v.traj)
        assert _row_values(m, v) == (before[k]["i"], before[k]["destpointer"], before[k]["force"])
        assert np.shares_memory(v._s, S) and np.shares_memory(v.znav, zn) and np.shares_memory(v.traj, m.ring)
        assert np.array_equal(v._s, S[v._index]) and np.array_equal(v.traj, m.ring[:, v._index].T)
    snapshot = [a.copy() for a in m.live()] + [m.ring.copy()]
    for k in (0, 3, 5):
        v = vs[k]
        assert v._mirror is None and _same(before[k], v)
        v._s += 1.0
        v.znav[:] = ~v.znav
        v.traj += 1.0
    assert all(np.array_equal(a, b) for a, b in zip(snapshot, list(m.live()) + [m.ring]))


@pytest.mark.parametrize("ticks", [3, 10])
def test_widening_keeps_contents_and_rebinds_views_at_each_class_width(ticks):
    """5 -> 6 states, before and after the ring has wrapped"""
    vs = [_Five(k, i=k % 2) for k in range(3)] + [_Car(3)]
    m = _mirror(vs)
    rng = np.random.default_rng(ticks)
    for _ in range(ticks):
        _tick(m, rng)
    seen = [_seen(v) for v in vs]
    rows = [_row_values(m, v) for v in vs]
    S_old, ring_old = m.live()[0].copy(), m.ring.copy()
    m.widen(6)
    S = m.live()[0]
    assert m.ns == 6 and S.shape == (4, 6) and m.ring.shape[::2] == (T, 6)
    assert np.array_equal(S[:, :5], S_old) and not S[:, 5].any()
    assert np.array_equal(m.ring[:, :, :5], ring_old) and not m.ring[:, :, 5].any()
    for v, was, row in zip(vs, seen, rows):
        assert v._s.shape == (type(v).N_STATES,) and np.shares_memory(v._s, S)
        assert np.array_equal(was["s"], v._s) and np.array_equal(was["znav"], v.znav) and np.array_equal(was["traj"], v.traj)
        assert np.shares_memory(v.traj, m.ring) != v.uncontrolled and v.traj.shape == (type(v).N_STATES, was["traj"].shape[1])
        assert _row_values(m, v) == row
    _adopt(m, [_Six(4)])                                               # the class the rows were widened for
    assert np.array_equal(m.vehicles[4]._s, m.live()[0][4]) and m.vehicles[4]._s.shape == (6,)


def test_ring_growth_keeps_earlier_columns_and_rebinds_earlier_views():
    first = [_Five(k) for k in range(2)]
    own = [v.traj.copy() for v in first]
    m = _mirror(first)
    assert m.ring.shape == (T, 2, 5)
    old_ring = m.ring
    more = [_Five(k, seed=1) for k in range(2, 5)]
    own += [v.traj.copy() for v in more]
    _adopt(m, more)
    assert m.ring is not old_ring and m.ring.shape == (T, 5, 5)        # max(n, 2 * rows)
    for k, v in enumerate(first + more):
        assert np.array_equal(m.ring[:, k].T, own[k]) and np.array_equal(v.traj, own[k])
        assert np.shares_memory(v.traj, m.ring) and not np.shares_memory(v.traj, old_ring)
    _adopt(m, [_Five(5, seed=2)])
    assert m.ring.shape == (T, 10, 5)                                  # geometric


def test_watching_starts_with_the_first_hand_out_and_names_exactly_the_edited_rows():
    vs = [_Five(k) for k in range(5)]
    m = _mirror(vs)
    rng = np.random.default_rng(0)
    _tick(m, rng)
    vs[1]._s[0] += 1.0                                                 # (a write nobody was told about: not looked for)
    assert not m.watched and m.changed_rows().size == 0
    shadow = m._shadow.copy()
    _tick(m, rng)
    assert np.array_equal(shadow, m._shadow)                           # no shadow copy per tick
    m.watch()                                                          # Vehicle.s: the hand-out comes before the write
    assert m.watched and m.changed_rows().size == 0
    vs[1]._s[0] += 1.0
    vs[3]._s[4] -= 2.0
    changed = m.changed_rows()
    assert changed.tolist() == [1, 3]
    assert np.array_equal(m.states(changed, 4), np.array([vs[1]._s[:4], vs[3]._s[:4]]))
    m.sync_shadow(changed)
    assert m.changed_rows().size == 0
    vs[2]._s[1] = 7.0
    _tick(m, rng)                                                      # a read-back: the device's view again
    assert m.changed_rows().size == 0


@pytest.mark.parametrize("n", [3, 513])
def test_adoption_of_one_class_goes_through_the_slabs(n):
    """uniform width: the slab copy, with more than one slab at 513"""
    vs = [_Five(k) for k in range(n)]
    own = [(v._s.copy(), v.traj.copy(), v.znav.copy(), v.i, v.destpointer, v.force) for v in vs]
    m = _mirror(vs, cap=n + 1)
    S, ptr, zn, fx, fy = m.live()
    assert S.shape == (n, 5) and m.ring.shape == (T, n, 5)
    for k, (v, (s, traj, znav, i, p, f)) in enumerate(zip(vs, own)):
        assert v._mirror is m and v._index == k
        assert np.array_equal(S[k], s) and np.array_equal(m._shadow[k], s) and np.array_equal(zn[k], znav) and m._vd[k] == k
        assert np.array_equal(m.ring[:, k].T, traj) and np.array_equal(v.traj, traj) and np.shares_memory(v.traj, m.ring)
        assert _row_values(m, v) == (i, p, f)


def test_adoption_of_mixed_widths_and_a_prescribed_trajectory():
    vs = [_Five(0), _Six(1), _Car(2), _Five(3)]
    script = vs[2].traj
    own = [v.traj.copy() for v in vs]
    m = _mirror(vs, ns=6)
    S = m.live()[0]
    for k, v in enumerate(vs):
        w = type(v).N_STATES
        assert np.array_equal(S[k, :w], v._s) and not S[k, w:].any() and v._s.shape == (w,)
        if v.uncontrolled:
            assert v.traj is script and np.array_equal(script, own[k]) and not m.ring[:, k].any()
        else:
            assert np.array_equal(m.ring[:, k, :w].T, own[k]) and not m.ring[:, k, w:].any()
            assert np.array_equal(v.traj, own[k]) and np.shares_memory(v.traj, m.ring)

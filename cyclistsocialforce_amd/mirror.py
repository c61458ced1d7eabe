"""`PopulationMirror`: the bulk host arrays behind the road users of one `SocialForceIntersection` and the books a tick leaves
in them.  NumPy only - no engine, no SUMO, nobody's drawing policy -, and nothing outside this module indexes its arrays.  A bound
vehicle is row `_index`: `vehicle.s`, `znav`, `traj` are views, `i`, `destpointer`, `force`, `F` read through `vehicle._mirror`."""
import numpy as np

FOLD_AT = 4096      # entries of the force log at which it is folded into the vehicles' own lists
SLAB = 512          # vehicles whose histories are adopted into the ring in one copy

_NO_ROWS = np.zeros(0, dtype=np.intp)


def _wider(a, ns):
    out = np.zeros(a.shape[:-1] + (ns,))
    out[..., : a.shape[-1]] = a
    return out


class PopulationMirror:
    def __init__(self):
        self.vehicles = []        # the bound vehicles: vehicle k is row k
        self._S = self._traj = None   # (allocate, grow_ring)
        self.have_force = False   # some tick's forces are in _fx / _fy
        self.watched = False      # some vehicle.s has been handed out: the state is compared with the shadow before every tick
        self.pos_stale = False    # the rows moved since the intersection last copied its vehicleX / Y / Theta
        self._flog = []           # |F| of every evaluated tick since the last fold (vehicle.F)
        self._flog_base = 0
        self._drawn = []          # vehicles with a drawing / saveForces (the only per-tick Python loop)
        self.drawn_stale = True

    # ------------------------------------------------------------------ the arrays
    def allocate(self, capacity, ns):
        self.ns = ns
        self._S = np.zeros((capacity, ns))              # state, as wide as the widest vehicle class; vehicle.s are row views
        self._shadow = np.zeros((capacity, ns))         # the device's view of _S after the last read-back / push, kept once `watched`
        self._vd = np.zeros(capacity)                   # v_desired
        self._ptr = np.zeros(capacity, dtype=np.int32)  # destpointer
        self._zn = np.zeros((capacity, 3), dtype=bool)  # vehicle.znav are row views
        self._fx, self._fy = np.zeros(capacity), np.zeros(capacity)
        self._ti = np.zeros(capacity, dtype=np.int64)   # vehicle.i: the ring column written last
        self._cls = np.zeros(capacity, dtype=np.int32)  # row of the parameter-set table
        # _traj, the ring [traj_len, rows, n_states] (a tick writes one contiguous slab; vehicle.traj are transposed views), comes
        # with the first vehicles: grow_ring

    @property
    def ring(self):
        return self._traj

    def widen(self, ns):
        """rows as wide as the widest vehicle class of the population"""
        self.ns, self._S, self._shadow = ns, _wider(self._S, ns), _wider(self._shadow, ns)
        if self._traj is not None:
            self._traj = _wider(self._traj, ns)
        self._rebind()

    def grow_ring(self, n, traj_len):
        """the ring with room for n rows of traj_len columns (grown geometrically; every vehicle of an engine shares t_s)"""
        rows = 0 if self._traj is None else self._traj.shape[1]
        if rows < n:
            grown = np.zeros((traj_len, max(n, 2 * rows), self.ns))
            if rows:
                grown[:, :rows] = self._traj
            self._traj = grown
            self._rebind()

    def live(self):
        """the rows of the bound vehicles (state, destination pointers, navigation state, Fx, Fy): one contiguous block of
        each, what a read-back straight into the mirror writes"""
        n = len(self.vehicles)
        return self._S[:n], self._ptr[:n], self._zn[:n], self._fx[:n], self._fy[:n]

    def store(self, s, ptr, zn, fx=None, fy=None):     # a read-back that did not go into the live rows
        n = len(self.vehicles)
        self._S[:n, : s.shape[1]] = s
        self._ptr[:n] = ptr
        self._zn[:n] = zn
        if fx is not None:
            self.store_forces(fx, fy)

    def store_forces(self, fx, fy):
        n = len(self.vehicles)
        self._fx[:n], self._fy[:n] = fx, fy                           # intersection.py:860-862
        self.have_force = True

    def positions(self):                        # copies of the x, y and psi columns
        S = self._S[: len(self.vehicles)]
        return S[:, 0].copy(), S[:, 1].copy(), S[:, 2].copy()

    # ------------------------------------------------------------------ vehicles come, stay and go
    def _views(self, v):                        # vehicle attributes that are views of the bulk arrays
        k, w = v._index, type(v).N_STATES       # (a mixed population: the rows are as wide as the widest class)
        v._s = self._S[k, :w]
        v.znav = self._zn[k]
        if not v.uncontrolled:                  # (an UncontrolledVehicle's traj is its prescription: vehicle.py:958-960)
            v.traj = self._traj[:, k, :w].T

    def _rebind(self):
        for v in self.vehicles:
            self._views(v)

    def bind(self, v):
        """row v._index is the vehicle's from now on: i, destpointer and force move into it"""
        k = v._index
        self._ti[k], self._ptr[k] = v.i, v.destpointer
        self._fx[k], self._fy[k] = v.force
        v._f_seen = self._flog_base + len(self._flog)
        v._mirror = self
        self._views(v)

    def detach(self, v):
        """the vehicle leaves with private copies of everything it saw through the mirror"""
        k = v._index
        i, ptr, force = int(self._ti[k]), int(self._ptr[k]), self.force_of(v) or v.force
        v._s, v.znav, v.traj = v._s.copy(), v.znav.copy(), v.traj.copy()
        v._mirror = None
        v.i, v.destpointer, v.force = i, ptr, force

    def adopt(self, new, s0, vd, traj_len):
        """The vehicles `new` take the rows behind the bound ones, with states s0 [len(new), ns] and desired speeds vd: state,
        shadow, v_desired and znav rows, their own histories [., traj_len] into the ring (a prescribed traj stays its
        vehicle's), parameter set 0 (where the engine starts a road user)."""
        first, m = len(self.vehicles), len(new)
        rows = slice(first, first + m)
        self.grow_ring(first + m, traj_len)
        self._S[rows] = self._shadow[rows] = s0
        self._vd[rows] = vd
        self._cls[rows] = 0
        if all(type(v).N_STATES == self.ns and not v.uncontrolled for v in new):
            for c in range(0, m, SLAB):         # a slab of rows at a time
                blk = new[c:c + SLAB]
                self._traj[:, first + c:first + c + len(blk), :] = np.stack([v.traj for v in blk]).transpose(2, 0, 1)
        else:
            for k, v in enumerate(new):
                if not v.uncontrolled:
                    self._traj[:, first + k, : type(v).N_STATES] = v.traj.T
        for k, v in enumerate(new):
            v._index = first + k
            self._zn[first + k] = v.znav
            self.bind(v)
        self.vehicles.extend(new)
        self.drawn_stale = True

    def compact(self, keep):
        """the rows `keep` (ascending) close up; the vehicles of the others are detached"""
        if not self.vehicles:
            return
        self.fold_all()                          # indices are about to change
        staying = set(keep)
        for k, v in enumerate(self.vehicles):
            if k not in staying:
                self.detach(v)
        m = len(keep)
        for a in (self._S, self._shadow, self._vd, self._ptr, self._zn, self._fx, self._fy, self._ti, self._cls):
            a[:m] = a[keep]
        if m:
            self._traj[:, :m] = self._traj[:, keep]
        self.vehicles = [self.vehicles[k] for k in keep]
        for k, v in enumerate(self.vehicles):
            v._index = k
            self._views(v)
        self.drawn_stale = True

    # ------------------------------------------------------------------ what a bound vehicle reads and writes
    def i_of(self, v):
        return int(self._ti[v._index])

    def set_i(self, v, value):
        self._ti[v._index] = value

    def pointer_of(self, v):
        return int(self._ptr[v._index])

    def set_pointer(self, v, value):
        self._ptr[v._index] = value

    def force_of(self, v):
        """total force of the last evaluated tick; None before there was one"""
        return (float(self._fx[v._index]), float(self._fy[v._index])) if self.have_force else None

    def set_force(self, v, force):
        self._fx[v._index], self._fy[v._index] = force

    # ------------------------------------------------------------------ edits: states, desired speeds, parameter sets
    def watch(self):
        """a vehicle.s view goes to the caller, who may write through it: from now on the state is compared with what the
        device holds (the shadow) before every tick"""
        if not self.watched:
            self._shadow[:] = self._S                                 # (nobody has written yet: the getter runs before the write)
            self.watched = True

    def sync_shadow(self, rows):
        self._shadow[rows] = self._S[rows]                            # (they were pushed: the device holds them)

    def changed_rows(self):                     # whose state was edited since the last sync; none while nobody watches
        if not self.watched:
            return _NO_ROWS
        n = len(self.vehicles)
        differ = self._S[:n] != self._shadow[:n]
        return np.where(differ.any(axis=1))[0] if differ.any() else _NO_ROWS

    def states(self, rows, ns):
        return self._S[rows][:, :ns]

    def update_v_desired(self, vd):             # of every row -> the rows where it is new
        ch = np.where(vd != self._vd[: vd.size])[0]
        self._vd[ch] = vd[ch]
        return ch

    def update_classes(self, cls):              # parameter-set row of the first cls.size rows -> the rows where it is new
        ch = np.where(cls != self._cls[: cls.size])[0]
        self._cls[: cls.size] = cls
        return ch

    # ------------------------------------------------------------------ the books behind a tick
    def drawn(self):                            # with a drawing or saveForces, listed anew when the population or a drawing changed
        if self.drawn_stale:
            self._drawn = [v for v in self.vehicles if v.drawing is not None or v.saveForces]
            self.drawn_stale = False
        return self._drawn

    def log_forces(self, fx, fy):
        """|F| of one tick [n] or of k ticks [k, n] (vehicle.F: logged as arrays, folded into a vehicle's list when it is read)"""
        mag = fx * fx                                                 # (np.hypot is three times the time of this at N = 16 384)
        mag += fy * fy
        np.sqrt(mag, out=mag)
        if mag.ndim == 2:
            self._flog.extend(mag)
        else:
            self._flog.append(mag)
        if len(self._flog) >= FOLD_AT:                                # (when the log is folded does not show in vehicle.F)
            self.fold_all()

    def book_tick(self, fx, fy, forces, advance):
        """behind one read-back into the live rows: the watched shadow, and if the tick counter moved (by `advance`) the force
        log, the ring, trajF and the drawings"""
        n = len(self.vehicles)
        if self.watched:
            self._shadow[:n] = self._S[:n]
        self.pos_stale = True
        if forces:
            self.have_force = True
        if not advance:
            return
        if forces:
            self.log_forces(fx, fy)
        # (the ring write is spelled here and in book_block: through one helper for both, a tick over hundreds of small
        #  intersections was 3 % behind - profiles/mirror_refactor_ab.txt)
        ti = self._ti[:n] = (self._ti[:n] + advance) % self._traj.shape[0]     # vehicle.py:1279-1282 (see DESIGN D5)
        if n and (ti == ti[0]).all():
            self._traj[ti[0], :n] = self._S[:n]                       # the usual case: everyone joined at tick 0
        else:
            self._traj[ti, np.arange(n)] = self._S[:n]
        for v in (self.drawn() if self.drawn_stale else self._drawn):
            k = v._index
            Fx, Fy = (fx[k], fy[k]) if forces else (0.0, 0.0)
            if v.saveForces:
                v.trajF[0, ti[k]] = Fx
                v.trajF[1, ti[k]] = Fy
            v.update_drawing(Fres=(Fx, Fy))

    def book_block(self, S, F):
        """book_tick(fx, fy, True, 1) behind each of K consecutive ticks at once, from their recorded states S [K, n, n_states]
        and total forces F [K, n, 2]: the ring, trajF, the force log and vehicle.i move as K read-backs would have moved them.
        K may exceed the ring: only the last rows survive, as with K single ticks.  (The live rows hold the last tick's values
        already; drawings want every tick on the host and do not come here.)"""
        n, K = len(self.vehicles), int(S.shape[0])
        if self.watched:
            self._shadow[:n] = self._S[:n]
        if K == 0:
            return
        self.pos_stale = self.have_force = True
        self.log_forces(F[:, :, 0], F[:, :, 1])
        T = self._traj.shape[0]
        k0 = max(0, K - T)                                            # (ticks before it are overwritten by later ones)
        ti0 = self._ti[:n].copy()
        steps = np.arange(k0 + 1, K + 1)
        w = S.shape[2]
        if n and (ti0 == ti0[0]).all():
            self._traj[(ti0[0] + steps) % T, :n, :w] = S[k0:]
        elif n:
            self._traj[(ti0[None, :] + steps[:, None]) % T, np.arange(n)[None, :], :w] = S[k0:]
        self._ti[:n] = (ti0 + K) % T                                  # vehicle.py:1279-1282 (see DESIGN D5)
        for v in (self.drawn() if self.drawn_stale else self._drawn):
            if v.saveForces:
                k = v._index
                cols = (ti0[k] + steps) % T
                v.trajF[0, cols] = F[k0:, k, 0]
                v.trajF[1, cols] = F[k0:, k, 1]

    def fold(self, v):                          # the log's entries the vehicle has not seen -> its own list
        start = v._f_seen - self._flog_base
        if start < len(self._flog):
            k = v._index
            v._F.extend(float(a[k]) for a in self._flog[start:])
            v._f_seen = self._flog_base + len(self._flog)

    def fold_all(self):
        if self._flog:
            for v in self.vehicles:
                self.fold(v)
        self._flog_base += len(self._flog)
        self._flog = []
        for v in self.vehicles:
            v._f_seen = self._flog_base

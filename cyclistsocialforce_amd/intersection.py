"""`SocialForceIntersection` and the road-element classes with the interface of
`cyclistsocialforce.intersection` (SocialForceIntersection :253-916, RoadEdge :214, RoadSegment :72,
Straight/CurvedRoadSegment :118/:149, RoadSegmentCollection :32), driving the HIP engine.

One `step()` is exactly one `csf_step(engine, 1)`: FOV mask, all-pairs repulsive field, clamp, destination
force, road-edge force, controller + kinematics for every vehicle, snapshot refresh — all on the GPU.
The Python objects are a mirror: user mutations of `vehicle.s`, `vehicle.params.v_desired_default`, the
destination queues or the population are pushed to the device before the next tick, and `vehicle.s`,
`traj`, `destpointer`, `znav`, `force`, `F` are refreshed after it.  `step_n(k)` runs k ticks without any
per-tick Python work.

SUMO co-simulation: with `activate_sumo_cosimulation=True` the intersection reads its footprint,
approach lanes and internal lanes from a sumolib-style `net`, finds arrivals and departures on its internal lanes
through TraCI, gives arriving road users a spline prototype across the junction, and pushes every position back with
`traci.vehicle.moveToXY` after each tick (intersection.py:341-453, 458-539, 679-688).  `traci` is imported on demand
or injected (`traci=`), so the seam is testable without a SUMO installation.  Arrivals and departures reach the device
incrementally (include/csf.h: csf_set_incremental).

`animate=True` gives every vehicle a `vizualisation.VehicleDrawing` on the axes passed in (intersection.py:881-885); the
drawings are refreshed from the host mirror after each tick's read-back.

Out of scope: populations mixing vehicle classes in one intersection, writing animation videos.
"""
import numpy as np

from . import _ffi, parameters
from .engine import Engine
from .mirror import PopulationMirror
from .parameters import RoadElementParameters
from .utils import angleSFMtoSUMO, generateSplinePrototype
from .vehicle import QUEUE_APPENDED, QUEUE_EDITED, QUEUE_RANK, QUEUE_REPLACED, Vehicle, vehicle_extents

PRIORITY_RULES = {"unregulated": _ffi.UNREGULATED, "p2r": _ffi.P2R}
DENSE_CHUNK = 512        # ticks per call of the dense paths = samples of the engines' rings (the bytes per member)
# why every tick of an intersection passes the host (SocialForceIntersection._host_reason)
EMPTY, HOOKS, POLES, DRAWN, FIRST_DRAWINGS = "empty", "force hooks", "drawn poles", "drawings or SUMO", "drawings on the first tick"


# ----------------------------------------------------------------------------- road elements

class RoadEdge:
    """intersection.py:214-250: a polyline whose vertices repel road users with -F_0 r^-sigma."""

    def __init__(self, vertices, params=None):
        self.vertices = np.asarray(vertices, dtype=float)
        self.params = params if params is not None else RoadElementParameters()

    def edges(self):
        return [self]

    def calcRepulsiveForce(self, x, y):
        """intersection.py:226-242: the force of this edge's vertices at the points (x, y), any common shape -> (Fx, Fy) of that shape.
        Evaluated on the device (Engine.field_map, road term) by a private engine that holds nothing but this edge; the engine
        is kept until the vertices or the parameters change.  A point exactly on a vertex gets nothing from that vertex."""
        x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
        verts = np.ascontiguousarray(self.vertices, dtype=float)
        sig = (verts.shape, verts.tobytes(), float(self.params.F_0), float(self.params.sigma))
        cache = self.__dict__.get("_field_cache")
        if cache is None or cache[0] != sig:
            if cache is not None:
                cache[1].close()
            eng = Engine(_road_probe_pod(), 1)
            eng.set_road(*flatten_road_elements([self]))
            cache = self._field_cache = (sig, eng)
        return cache[1].field_map(x, y, crowd=False, road=True)


def _road_probe_pod():
    """the parameter set of an engine that holds a road and no road user (RoadEdge.calcRepulsiveForce): any vehicle class's defaults"""
    return parameters.BicycleParameters().to_pod(_ffi.TWOD)


def _sum_repulsive_force(parts, x, y):
    """intersection.py:36-48, 81-94: the parts' forces at the flattened points, added up part by part, in the shape of x"""
    x, y = np.asarray(x, dtype=float), np.asarray(y, dtype=float)
    shape = x.shape
    x, y = x.flatten(), y.flatten()
    Fx, Fy = np.zeros_like(x), np.zeros_like(y)
    for part in parts:
        fx, fy = part.calcRepulsiveForce(x, y)
        Fx += fx
        Fy += fy
    return np.reshape(Fx, shape), np.reshape(Fy, shape)


class RoadSegment:
    """intersection.py:72-115: two edges at +-width/2 around a centre line starting at x0 = (x, y, heading).
    As in the reference the segment's own `params` are defaults; the edges carry the ones passed in."""

    def __init__(self, x0, width, ds=0.1, params=None):
        self.params = RoadElementParameters()
        self.x0 = x0
        self.x1 = x0
        self.width = width
        self.edge_list = []
        self.ds = ds

    def edges(self):
        return list(self.edge_list)

    def calcRepulsiveForce(self, x, y):
        """intersection.py:81-94: the sum of the two edges' forces"""
        return _sum_repulsive_force(self.edge_list, x, y)

    @staticmethod
    def _place(local_xy, origin, heading):
        c, s = np.cos(heading), np.sin(heading)
        rot = np.array([[c, -s], [s, c]])
        return (rot @ np.asarray(local_xy, dtype=float).T).T + np.asarray(origin[:2], dtype=float)


class StraightRoadSegment(RoadSegment):
    """intersection.py:118-146: vertices every `ds` along a straight of `length`."""

    def __init__(self, x0, width, length, ds=0.1, params=None):
        RoadSegment.__init__(self, x0, width, ds, params)
        params = params if params is not None else RoadElementParameters()
        self.length = length
        along = np.arange(0, length + self.ds, self.ds)                # :126
        for side in (-0.5, 0.5):                                       # right edge first (:127-140)
            local = np.c_[along, np.full_like(along, side * width)]
            self.edge_list.append(RoadEdge(self._place(local, x0, x0[2]), params=params))
        self.x1 = np.zeros_like(np.asarray(x0, dtype=float))           # :142-146
        self.x1[:2] = np.asarray(x0[:2], dtype=float) + length * np.array([np.cos(x0[2]), np.sin(x0[2])])
        self.x1[2] = x0[2]


class CurvedRoadSegment(RoadSegment):
    """intersection.py:149-211: circular arc of `radius` through `angle`, turning "left" or "right"."""

    def __init__(self, x0, width, radius, angle, direction, ds=0.1, params=None):
        RoadSegment.__init__(self, x0, width, ds, params)
        params = params if params is not None else RoadElementParameters()
        assert direction in ("left", "right"), f'direction has to be "left" or "right, instead it was {direction}'
        self.length = radius * angle
        self.radius, self.angle, self.direction = radius, angle, direction
        turn = 1 if direction == "left" else -1                        # :166
        beta = x0[2] - np.pi / 2                                       # :173
        for sign in (+1, -1):                                          # right edge first (:176-207)
            r_edge = radius + sign * turn * width / 2
            grid = np.linspace(0, angle, int(r_edge * angle / self.ds))
            local = np.c_[turn * (r_edge * np.cos(grid) - radius), r_edge * np.sin(grid)]
            self.edge_list.append(RoadEdge(self._place(local, x0, beta), params=params))
        end_local = np.array([[turn * (radius * np.cos(angle) - radius), radius * np.sin(angle)]])
        self.x1 = np.zeros(3)                                          # :209-211
        self.x1[:2] = self._place(end_local, x0, beta)[0]
        self.x1[2] = x0[2] + turn * angle


class RoadSegmentCollection:
    """intersection.py:32-69"""

    def __init__(self, segs):
        self.segs = segs

    def edges(self):
        return [e for seg in self.segs for e in seg.edges()]

    def calcRepulsiveForce(self, x, y):
        """intersection.py:36-48: the sum of the segments' forces (scenarios/curve-scenario.py:90-125 maps it on a meshgrid)"""
        return _sum_repulsive_force(self.segs, x, y)

    def get_destinations_from_segments(self):
        return [seg.x1[0] for seg in self.segs], [seg.x1[1] for seg in self.segs]

    def __getitem__(self, i):
        if not isinstance(i, int):
            raise ValueError("Subscription index must be integer!")
        if i > len(self.segs):
            raise IndexError(f"RoadSegmentCollection has {len(self.segs)} segments, but i={i} was requested")
        return self.segs[i]


def flatten_road_elements(elements):
    """(offsets[n_edges+1], vertices[sum,2], F0[n_edges], sigma[n_edges]) of a road_elements list."""
    edges = [e for el in elements for e in el.edges()]
    off = np.zeros(len(edges) + 1, dtype=np.int64)
    for k, e in enumerate(edges):
        off[k + 1] = off[k] + e.vertices.shape[0]
    verts = np.vstack([e.vertices for e in edges]) if edges else np.zeros((0, 2))
    return off, verts, np.array([e.params.F_0 for e in edges]), np.array([e.params.sigma for e in edges])


# ----------------------------------------------------------------------------- the population tick

class SocialForceIntersection:
    """Open space / intersection managing one population of road users (intersection.py:253-916)."""

    def __init__(self, vehicleList, id="", priority_rule="unregulated", animate=False, axes=None,
                 activate_sumo_cosimulation=False, net=None, road_elements=[], bicycle_drawing_kwargs={},
                 capacity=None, device=0, track_params=True, traci=None):
        if animate and axes is None:
            raise AssertionError("Provide axes for animation!")        # intersection.py:409
        if priority_rule not in PRIORITY_RULES:
            raise ValueError(f"priority_rule must be one of {tuple(PRIORITY_RULES)}")
        assert isinstance(id, str), "Intersection ID has to be a string."
        self.bicycle_drawing_kwargs = bicycle_drawing_kwargs
        self.is_first_step = True
        self.activate_sumo_cosimulation = bool(activate_sumo_cosimulation)
        self._traci = traci
        self.id = id
        self.priority_rule = priority_rule
        self.animate = bool(animate)
        self.ax = axes
        self.road_elements = road_elements
        self.hist_n_vecs = []
        self.vehicles = []
        self.n_bikes = 0
        self._vx = np.zeros((0, 1))       # vehicleX / vehicleY / vehicleTheta (intersection.py:660-677): refreshed when read
        self._vy = np.zeros((0, 1))
        self._vth = np.zeros((0, 1))
        self._device = device
        self._capacity = capacity
        self._track_params = track_params
        self._engine = None
        self._small_classes = None   # set_small_classes: what the engine is told once it exists (None: the engine's own default)
        self._mid_road = None        # set_mid_road: the same
        self._mid_classes = None     # set_mid_classes: the same
        self._mirror = PopulationMirror()   # the bulk host arrays of the per-vehicle attributes the device produces, and their books
        self._scripted = []       # live UncontrolledVehicles (their traj may be rewritten while they run)
        self._rule_on_device = None
        self._class_table = None
        self._road_sig = None
        self._pending = []        # vehicles waiting to be added to the engine
        self._hooked = False      # some vehicle carries a custom rep_force_func / dest_force_func: forces are formed on the host (_hooked_forces)
        self._field_engines = {}  # ... engines for the class fields of the others, by parameter set
        self._stoch, self._stoch_for, self._stoch_epoch = [], -1, 0   # riders with stochastic_control_behavior (cache)
        self._dirty_queues = {}   # vehicle -> QUEUE_APPENDED | QUEUE_REPLACED | QUEUE_EDITED
        self._params_seen = -1
        if self.activate_sumo_cosimulation:
            self._init_sumo(net)
        for v in vehicleList:                                  # (as given: the reference plans no route for them, :316-317)
            self._attach(v)
        if self.activate_sumo_cosimulation:
            self.update_road_user_positions()                  # intersection.py:320

    # ------------------------------------------------------------------ SUMO co-simulation
    def _init_sumo(self, net):
        """intersection.py:341-405: footprint, the last / first two points of every approach / exit lane (sampled from
        a spline through the lane shape), and the internal lanes on which SUMO hands road users over."""
        from scipy import interpolate

        if net is None:
            raise ValueError("activate_sumo_cosimulation=True needs the sumolib net of the scenario (net=...)")
        if self._traci is None:
            try:
                import traci as _traci
            except ImportError as exc:
                raise ImportError("SUMO co-simulation needs the `traci` package (or pass traci=...)") from exc
            self._traci = _traci
        self.node = net.getNode(self.id)
        self.shape_vertices = np.asarray(self.node.getShape(), dtype=float)
        try:
            from matplotlib import path as pth
            self.shape = pth.Path(self.shape_vertices, closed=True)
        except ImportError:                                   # pragma: no cover - matplotlib is optional
            self.shape = self.shape_vertices

        def lane_ends(edges, order, take):
            ends = {}
            for edge in edges:
                ends[edge.getID()] = []
                for lane in edge.getLanes():
                    path = np.asarray(lane.getShape(), dtype=float)
                    tck, _ = interpolate.splprep((path[:, 0], path[:, 1]), s=0.0, k=min(order, path.shape[0] - 1))
                    x_i, y_i = interpolate.splev(np.linspace(0, 1, 10), tck)
                    ends[edge.getID()].append((x_i[take], y_i[take]))
            return ends

        self.inEdges = lane_ends(self.node.getIncoming(), 5, slice(-2, None))
        self.outEdges = lane_ends(self.node.getOutgoing(), 3, slice(None, 2))
        self.internal_lanes, self.internal_lane_ids = [], []
        for edge in net.getEdges():
            if edge.getFromNode() == self.node and edge.getToNode() == self.node:
                for lane in edge.getLanes():
                    self.internal_lane_ids.append(lane.getID())
                    self.internal_lanes.append(lane)
        if not self.internal_lanes:
            raise ValueError(f"Intersection {self.id} does not have internal lanes! Cyclistsocialforce requires internal "
                             "lanes to allocate SUMO road users to intersections. Check if the net-file correctly "
                             "specifies interal lanes for this intersection!")

    def find_entered_exited_roadusers(self):
        """intersection.py:429-453: ids that appeared on / vanished from the internal lanes during the last SUMO step."""
        before = self.get_road_user_ids()
        now = []
        for lane in self.internal_lane_ids:
            now += list(self._traci.lane.getLastStepVehicleIDs(lane))
        return np.setdiff1d(now, before), np.setdiff1d(before, now)

    def _route_prototype(self, user):
        """intersection.py:471-519: destinations across the junction for a road user that follows a SUMO route."""
        ecurrent, enext = user.route[0], user.route[1]
        assert ecurrent in self.inEdges, f"Road user {user.id} arriving on junction {self.id} from unknown edge {ecurrent}!"
        assert enext in self.outEdges, f"Road user {user.id} requesting to depart junction {self.id} on unknown edge {enext}!"
        lanes_in = self.inEdges[ecurrent]
        lane_in = 0
        if len(lanes_in) > 1:                                  # the closer of the first two approach lanes
            xs = np.concatenate((lanes_in[0][0], lanes_in[1][0]))
            ys = np.concatenate((lanes_in[0][1], lanes_in[1][1]))
            lane_in = int(np.argmin(np.hypot(xs - user._s[0], ys - user._s[1])) / 2)
        lane_out = np.random.randint(0, len(self.outEdges[enext]))
        pts = np.vstack((np.array(lanes_in[lane_in]).T, np.array(self.outEdges[enext][lane_out]).T))
        xp, yp = generateSplinePrototype(pts[:, 0], pts[:, 1], 5)
        ahead = np.hypot(xp - xp[-1], yp - yp[-1]) < np.hypot(user._s[0] - xp[-1], user._s[1] - yp[-1])
        user.setDestinations(xp[ahead], yp[ahead], reset=True)  # only the points still in front of the road user

    # ------------------------------------------------------------------ population management
    def _attach(self, v):
        if not isinstance(v, Vehicle):
            raise TypeError("road users must be cyclistsocialforce_amd.vehicle.Vehicle objects")
        if v._owner is not None and v._owner is not self:
            raise RuntimeError(f"vehicle {v.id} already belongs to another intersection")
        self._stoch_for = -1
        if v.dest_force_func is not None or v.rep_force_func is not None:
            self._hooked = True                                        # (this population's forces are formed on the host: _hooked_forces)
        if v._solo is not None:
            v._solo.close()
            v._solo = None
        v._owner = self
        v._index = len(self.vehicles)
        v._queue_synced = -1
        self._dirty_queues[v] = QUEUE_REPLACED
        self.vehicles.append(v)
        self._pending.append(v)
        self.n_bikes = len(self.vehicles)
        self._mirror.pos_stale = True                                         # intersection.py:531-538: vehicleX ... grow by a row

    def _param_classes(self, vehicles=None):
        """The parameter sets of the population.  Every reference vehicle owns its params object: the field vehicle i
        exerts is evaluated with ITS f_0 / sigma / e (vehicle.py:1592-1612) and masked with ITS hfov
        (intersection.py:733-735), and it moves with its own gains and limits.  The engine holds a table of up to 256
        distinct csf_params and a row index per road user (csf_set_param_classes); `params.v_desired_default` is per
        road user anyway.  Returns (list of PODs, vehicle 0's first; int32 row of every vehicle)."""
        vehicles = self.vehicles if vehicles is None else vehicles
        rule = PRIORITY_RULES.get(self.priority_rule, 0)
        by_object, rows, pods = {}, {}, []
        cls = np.zeros(len(vehicles), dtype=np.int32)
        for k, v in enumerate(vehicles):
            c = by_object.get(id(v.params))
            if c is None:
                pod = v._pod(rule)
                key = bytes(pod)
                c = rows.get(key)
                if c is None:
                    if pods and (pod.t_s != pods[0].t_s or pod.traj_len != pods[0].traj_len):
                        raise NotImplementedError(f"vehicle {v.id!r}: t_s = {pod.t_s} but vehicle {vehicles[0].id!r} has "
                                                  f"{pods[0].t_s}; the road users of one intersection share the clock")
                    c = rows[key] = len(pods)
                    pods.append(pod)
                by_object[id(v.params)] = c
            cls[k] = c
        if len(pods) > 256:
            raise NotImplementedError(f"{len(pods)} distinct parameter sets in one intersection; the engine's table holds 256")
        return pods, cls

    def _sync_param_classes(self):
        """table and rows -> engine, when they changed (new road users, assignments to parameter attributes)"""
        pods, cls = self._param_classes()
        self._sync_param_table(pods, cls, len(self.vehicles))
        self._sync_param_rows(cls)

    def _sync_param_table(self, pods, cls, n_on_device):
        e = self._engine
        table = tuple(bytes(p) for p in pods)
        if table != self._class_table:
            if self._class_table is not None and len(table) < len(self._class_table) and n_on_device:
                e.set_agent_class(np.arange(n_on_device), cls[:n_on_device])      # rows first: none may point beyond the new table
                self._mirror.update_classes(cls[:n_on_device])
            e.set_param_classes(pods)
            self._class_table = table

    def _sync_param_rows(self, cls):
        ch = self._mirror.update_classes(cls)
        if ch.size:
            self._engine.set_agent_class(ch, cls[ch])

    def add_road_user(self, user):
        """intersection.py:458-539"""
        if self.activate_sumo_cosimulation and user.follow_route:
            self._route_prototype(user)
        if self.animate:                                       # intersection.py:521-524
            if user.drawing is None:
                user.add_drawing(self.ax, **self.bicycle_drawing_kwargs)
            user.drawing.set_animated(True)
        self._attach(user)

    def get_road_user_ids(self):
        return [v.id for v in self.vehicles]

    def has_road_user(self, userId):
        assert isinstance(userId, str), "User ID has to be a string."
        return userId in self.get_road_user_ids()

    def remove_road_user(self, i_remove):
        """intersection.py:618-634"""
        self._remove([int(i_remove)])

    def remove_road_users_by_id(self, ruids):
        """intersection.py:576-616"""
        idx = [k for k, v in enumerate(self.vehicles) if v.id in ruids]
        if idx:
            self._remove(idx)

    def _remove(self, idx):
        idx = sorted(set(idx))
        self._stoch_for = -1
        for k in idx:
            if not 0 <= k < len(self.vehicles):
                raise IndexError(f"no road user {k}")
        if self._engine is not None:
            self._flush_pending()
            self._engine.remove_agents(idx)
        gone = set(idx)
        keep = [k for k in range(len(self.vehicles)) if k not in gone]
        self._mirror.compact(keep)                   # (the leavers take private copies of what they saw through it)
        for k in idx:
            v = self.vehicles[k]
            v._owner, v._index = None, -1
            if v in self._pending:
                self._pending.remove(v)
            self._dirty_queues.pop(v, None)
        self.vehicles = [self.vehicles[k] for k in keep]
        for new, v in enumerate(self.vehicles):
            v._index = new
        self._scripted = [v for v in self._scripted if v._owner is self]
        self.n_bikes = len(self.vehicles)
        self._mirror.pos_stale = True

    def addEdge(self, roadEdge):
        self.road_elements.append(roadEdge)

    # ------------------------------------------------------------------ host <-> device mirror
    def _engine_ready(self):
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        if self._engine is None:
            pod = self.vehicles[0]._pod(PRIORITY_RULES[self.priority_rule])
            cap = self._capacity or max(256, 4 * len(self.vehicles))
            self._engine = Engine(pod, cap, device=self._device)
            if self._small_classes is not None:
                self._engine.small_classes(self._small_classes)
            if self._mid_road is not None:
                self._engine.mid_road(self._mid_road)
            if self._mid_classes is not None:
                self._engine.mid_classes(self._mid_classes)
            self._capacity = cap
            self._mirror.allocate(cap, max(type(v).N_STATES for v in self.vehicles))
            self._rule_on_device = self.priority_rule
            self._class_table = (bytes(pod),)
        self._flush_pending()
        return self._engine

    def _flush_pending(self):
        if not self._pending:
            return
        e, m = self._engine, self._mirror
        if len(self.vehicles) > self._capacity:
            raise RuntimeError(f"intersection capacity {self._capacity} exceeded; pass capacity= at construction")
        new = self._pending
        self._pending = []
        pods, cls = self._param_classes()                      # of everyone, the arrivals included
        ns = max(m.ns, max(type(v).N_STATES for v in new))
        if ns > m.ns:                                          # a wider vehicle class joins: wider rows
            m.widen(ns)
        self._sync_param_table(pods, cls, len(self.vehicles) - len(new))   # first: it decides the engine's state layout
        s0 = np.zeros((len(new), ns))
        for k, v in enumerate(new):
            s0[k, : v._s.size] = v._s
        vd = np.array([float(getattr(v.params, "v_desired_default", 0.0)) for v in new])   # (CarParameters have none)
        e.add_agents(s0[:, : e.ns], vd)
        scripted = [v for v in new if v.uncontrolled]
        if scripted:
            self._send_scripts(e, scripted)
            self._scripted.extend(scripted)
        T = int(30 / new[0].params.t_s)                        # vehicle.py:159
        for v in new:
            if v.traj.shape[1] != T and not v.uncontrolled:
                raise NotImplementedError("all road users of one intersection share t_s (one engine per intersection)")
        m.adopt(new, s0, vd, T)
        self._dirty_queues.update(dict.fromkeys(new, QUEUE_REPLACED))
        self._sync_param_rows(cls)

    def _mark_queue_dirty(self, v, how):
        """how: QUEUE_APPENDED, QUEUE_REPLACED (the pointer rewinds) or QUEUE_EDITED (in place, the pointer is kept)"""
        prev = self._dirty_queues.get(v, QUEUE_APPENDED)
        self._dirty_queues[v] = how if QUEUE_RANK[how] >= QUEUE_RANK[prev] else prev

    def _push_mutations(self):
        """Everything the user may have changed on the Python side since the last tick."""
        e = self._engine
        if e is None or self._pending or not self.vehicles:
            e = self._engine_ready()
        if self._scripted:                       # (each step behind the test that says whether it has anything to look at: a tick of
            self._push_scripts(e)                #  a population nobody touched makes none of these calls)
        if self._dirty_queues:
            self._push_queues(e)
        if self._mirror.watched:
            self._push_states(e)
        if self._track_params and parameters.mutation_count() != self._params_seen:
            self._push_params(e)
        if self.priority_rule != self._rule_on_device:
            self._push_rule(e)
        if tuple(id(el) for el in self.road_elements) != self._road_sig:
            self._push_road(e)
        return e

    # UncontrolledVehicle: the reference reads car.traj[:, i] on every step (vehicle.py:964-979), so a trajectory written
    # after the car joined - external control - has to reach the engine: compare with what was sent, send again on a change
    def _push_scripts(self, e):
        changed = []
        for v in self._scripted:
            if v._mirror is not None and getattr(v, "_script_sent", None) is not None:
                cur = np.ascontiguousarray(v.traj.T)
                if cur.shape != v._script_sent.shape or not np.array_equal(cur, v._script_sent):
                    v._script = cur
                    changed.append(v)
        if changed:
            self._send_scripts(e, changed)

    def _send_scripts(self, e, cars):
        """prescribed trajectories -> the engine (csf_set_script), and what it holds now is remembered: later writes to car.traj are noticed"""
        rows = [v._script if v._script is not None else np.zeros((0, 4)) for v in cars]
        e.set_script([v._index for v in cars], np.cumsum([0] + [r.shape[0] for r in rows]), np.vstack(rows))
        for v in cars:
            v._script_sent = np.ascontiguousarray(v.traj.T).copy()

    # destination queues (only vehicles whose setDestinations / stop / go ran since the last push): replaced queues go up
    # first, then the ones edited in place, then appended rows
    def _push_queues(self, e):
        groups = {mode: ([], [], [0]) for mode in (QUEUE_REPLACED, QUEUE_EDITED, QUEUE_APPENDED)}
        for v, how in self._dirty_queues.items():
            rows = v.destqueue
            mode = QUEUE_REPLACED if v._queue_synced < 0 else how
            if mode == QUEUE_APPENDED:
                if v._queue_synced >= rows.shape[0]:
                    continue
                rows = rows[v._queue_synced:]
            agents, blocks, off = groups[mode]
            agents.append(v._index); blocks.append(rows); off.append(off[-1] + rows.shape[0])
            v._queue_synced = v.destqueue.shape[0]
            v._queue_dirty = False
        self._dirty_queues = {}
        for mode, (agents, blocks, off) in groups.items():
            if agents:
                e.set_dest_queue(agents, off, np.vstack(blocks), reset=mode)

    # vehicle.s edited in place (calibration.py:455-460): looked for once a vehicle.s has been handed out (Vehicle.s)
    def _push_states(self, e):
        changed = self._mirror.changed_rows()
        if changed.size:
            e.push_state(changed, self._mirror.states(changed, e.ns))
            self._mirror.sync_shadow(changed)

    # params.v_desired_default is the per-agent parameter (demoCSFstandalone.py:104-113); the population is rescanned
    # only after some parameter object was assigned to
    def _push_params(self, e):
        self._params_seen = parameters.mutation_count()
        vd = np.array([float(getattr(v.params, "v_desired_default", 0.0)) for v in self.vehicles])
        ch = self._mirror.update_v_desired(vd)
        if ch.size:
            e.set_v_desired(ch, vd[ch])
        self._sync_param_classes()

    def _push_rule(self, e):
        if self.priority_rule not in PRIORITY_RULES:
            raise ValueError(f"priority_rule must be one of {tuple(PRIORITY_RULES)}")
        e.set_priority_rule(PRIORITY_RULES[self.priority_rule])
        self._rule_on_device = self.priority_rule

    def _push_road(self, e):
        e.set_road(*flatten_road_elements(self.road_elements))
        self._road_sig = tuple(id(el) for el in self.road_elements)

    def _pull(self, forces=True, advance=1, step=0):
        """One read-back of the device's view into the bulk mirror (vehicle.s, znav, traj are views of it); step: that many
        ticks first, in the same call (csf_step_get_tick)."""
        e, m = self._engine, self._mirror
        if step and m.ns == e.ns:
            S, ptr, zn, fx, fy = m.live()
            if not forces:
                fx = fy = None
            e.step_into(step, S, ptr, zn, fx, fy)
        else:
            s, ptr, zn, fx, fy, _ = e.step_snapshot(step, forces=forces, reuse=True) if step else e.tick_snapshot(forces=forces)
            m.store(s, ptr, zn, fx if forces else None, fy)
        return self._book_tick(fx, fy, forces, advance)

    def _book_tick(self, fx, fy, forces, advance):
        """the host's per-tick bookkeeping behind a read-back into the bulk mirror (_pull; step_together): the mirror's books,
        and SUMO is told every tick (else the positions are refreshed when somebody reads them)"""
        self._mirror.book_tick(fx, fy, forces, advance)
        if self.activate_sumo_cosimulation:
            self.update_road_user_positions()
        return fx, fy

    def _book_block(self, S, F):
        """behind a chunk of recorded ticks whose last read-back went straight into the live rows (step_n(dense=True),
        advance_together): what that many calls of step() leave on the host (drawings and SUMO want every tick on the host and
        do not come here: _dense_engine)"""
        self.is_first_step = False
        self._mirror.book_block(S, F)
        self.hist_n_vecs.extend([self.n_bikes] * int(S.shape[0]))

    # vehicleX / vehicleY / vehicleTheta (intersection.py:660-677) are refreshed when they are read: three column copies of the
    # mirror per tick are a tenth of the tick's host time at N = 16 384, and most ticks nobody looks
    def _positions(self):
        if self._mirror.pos_stale:
            self.update_road_user_positions()
        return self._vx, self._vy, self._vth

    vehicleX = property(lambda self: self._positions()[0], lambda self, a: setattr(self, "_vx", a))
    vehicleY = property(lambda self: self._positions()[1], lambda self, a: setattr(self, "_vy", a))
    vehicleTheta = property(lambda self: self._positions()[2], lambda self, a: setattr(self, "_vth", a))

    def update_road_user_positions(self):
        """intersection.py:660-677"""
        n = len(self.vehicles)
        self._mirror.pos_stale = False
        if self._vx.shape[0] != n:
            self._vx, self._vy, self._vth = np.zeros((n, 1)), np.zeros((n, 1)), np.zeros((n, 1))
        if n and len(self._mirror.vehicles) == n:                  # (everyone is bound)
            self._vx[:, 0], self._vy[:, 0], self._vth[:, 0] = self._mirror.positions()
        else:
            for k, v in enumerate(self.vehicles):
                self._vx[k, 0], self._vy[k, 0], self._vth[k, 0] = v._s[0], v._s[1], v._s[2]
        if self.activate_sumo_cosimulation and n:              # intersection.py:679-688: SUMO follows the social-force positions
            move = self._traci.vehicle.moveToXY
            angles = angleSFMtoSUMO(self.vehicleTheta[:, 0])
            for k, v in enumerate(self.vehicles):
                move(v.id, "", -1, float(self.vehicleX[k, 0]), float(self.vehicleY[k, 0]), angle=float(angles[k]), keepRoute=6)

    # ------------------------------------------------------------------ reference API
    def get_untracked_foes(self):
        """intersection.py:690-745: boolean [n, n], True where a road user is not considered.  As in the reference the
        first index is the road user whose force field is evaluated (the source, whose hfov applies: :733-735) and the
        second the one that would feel it; the diagonal is True, and a single road user yields `np.array(True)`."""
        if self.n_bikes <= 1:
            return np.array((True))
        return self._push_mutations().untracked()

    def calc_forces(self):
        """intersection.py:747-864: total force on every road user from the current snapshot."""
        e = self._push_mutations()
        if self._hooked and self.n_bikes > 0:
            fx, fy = self._hooked_forces(e)
            self._mirror.store_forces(fx, fy)
        else:
            fx, fy = e.calc_forces()
            self._pull(forces=True, advance=0)
        self._mirror.log_forces(fx, fy)
        return fx, fy

    def force_field(self, X, Y, psi=0.0, crowd=True, road=True, fov=False, exclude=None):
        """The force field of the live population and of `road_elements` at the probe points (X, Y), any common shape -> (Fx, Fy)
        of that shape: what a road user of heading psi (a scalar, or an array of that shape) would feel there - the sum of every
        road user's calcRepulsiveForce (its class's field, its own parameter set; unclamped: limitMagnitude needs a destination
        force, which a probe has not) and the road-edge term.  fov: the probe ignores the road users a receiver there would ignore
        (get_untracked_foes, the priority rule included).  exclude: a vehicle of this intersection, or its id, left out as a source -
        what THAT rider would feel elsewhere.  One launch per term on the population's own engine (Engine.field_map)."""
        X, Y = np.asarray(X, dtype=float), np.asarray(Y, dtype=float)
        if crowd and any(v.rep_force_func is not None for v in self.vehicles):
            raise NotImplementedError("force_field: a vehicle carries a custom rep_force_func - that field lives in Python")
        left_out = None
        if exclude is not None:
            hit = [v for v in self.vehicles if v is exclude or (not isinstance(exclude, Vehicle) and v.id == exclude)]
            if not hit:
                raise ValueError(f"force_field: {exclude!r} is no road user of this intersection")
            left_out = hit[0]
        if not self.vehicles:                                      # nobody there: the road elements' own engines
            if X.shape != Y.shape:
                raise ValueError(f"force_field: X {X.shape} and Y {Y.shape} differ in shape")
            if road:
                return _sum_repulsive_force(self.road_elements, X, Y)
            return np.zeros(X.shape), np.zeros(X.shape)
        e = self._push_mutations()
        skip = -1 if left_out is None else left_out._index        # (its place in the population order, once arrivals are on the device)
        return e.field_map(X, Y, psi, crowd=crowd, road=road, fov=fov, skip=skip)

    def encounters(self, first=None, count=None, radius=0.5, d_event=None, ttc_event=None, per_sample=True):
        """Engine.encounters on the population's own engine: closest approach and time to collision of every road user, each a disc
        of `radius`, over samples [first, first + count) of the engine's recording (step_n(..., dense=True) and advance_together
        record every tick in a ring of DENSE_CHUNK samples) or - first=None - now.  The result carries the partners also as the road
        users' ids: `ids`, d_with_id, ttc_with_id [count, n] and run_d_with_id, run_ttc_with_id [n] (None where there is no partner).  A window that begins before the
        ring was started, or before road users last came, went or were swapped, is refused: the recording begins a new stretch then
        (csf.h, "the lifetime of a recording")."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        return _encounter_ids(self._push_mutations().encounters(first, count, radius, d_event, ttc_event, per_sample), self.get_road_user_ids())

    def post_encroachment(self, first, count, pet_event=None, per_segment=True):
        """Engine.post_encroachment on the population's own engine: who crossed whose path, where, and how long after the other had
        passed, over samples [first, first + count) of the engine's recording (step_n(..., dense=True) and advance_together record
        every tick in a ring of DENSE_CHUNK samples).  The result carries the partners also as the road users' ids: `ids`,
        seg_with_id [count - 1, n], run_with_id [n] (None where there is no partner) and event_i_id, event_j_id beside the events.  A window that begins before the
        ring was started, or before road users last came, went or were swapped, is refused: the recording begins a new stretch then
        (csf.h, "the lifetime of a recording")."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        return _pet_ids(self._push_mutations().post_encroachment(first, count, pet_event, per_segment), self.get_road_user_ids())

    def passing(self, first, count, band=0.75, lat_max=3.0, lat_event=None, per_station=True):
        """Engine.passing on the population's own engine: who rode behind whom, at what gap and headway, and who overtook or met
        whom, when and at what lateral clearance, over samples [first, first + count) of the engine's recording (step_n(...,
        dense=True) and advance_together record every tick in a ring of DENSE_CHUNK samples).  The result carries the partners also
        as the road users' ids: `ids`, gap_with_id [count - 1, n], made_with_id, by_with_id [count - 2, n], run_gap_with_id,
        run_thw_with_id, run_made_with_id, run_by_with_id [n] (None where there is no partner) and event_i_id, event_j_id beside the
        events.  A window that begins before the
        ring was started, or before road users last came, went or were swapped, is refused: the recording begins a new stretch then
        (csf.h, "the lifetime of a recording")."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        return _passing_ids(self._push_mutations().passing(first, count, band, lat_max, lat_event, per_station), self.get_road_user_ids())

    def flow(self, first, count, lines=None, areas=None, grid=None, events=False):
        """Engine.flow on the population's own engine: the crossings of counting lines, the occupancy of areas and of a grid, over
        samples [first, first + count) of the engine's recording (step_n(..., dense=True) and advance_together record every tick in
        a ring of DENSE_CHUNK samples).  The result carries the road users' ids: `ids` - row i of cross_n, first_* and in_* is
        ids[i] - and event_i_id beside the events.  A window that begins before the
        ring was started, or before road users last came, went or were swapped, is refused: the recording begins a new stretch then
        (csf.h, "the lifetime of a recording")."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        return _flow_ids(self._push_mutations().flow(first, count, lines, areas, grid, events), self.get_road_user_ids())

    def clearance(self, first, count, road=None, d_event=0.0, events=False, per_sample=True):
        """Engine.clearance on the population's own engine: the distances to, the sides of and the crossings of the edges of a road,
        over samples [first, first + count) of the engine's recording (step_n(..., dense=True) and advance_together record every
        tick in a ring of DENSE_CHUNK samples).  road=None: the intersection's own road_elements (a ValueError if it has none).  The
        result carries the road users' ids: `ids` - row i of the per-road-user arrays is ids[i] - and event_i_id beside the events.
        A window that begins before the ring was started, or before road users last came, went or were swapped, is refused: the
        recording begins a new stretch then (csf.h, "the lifetime of a recording")."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        if road is None:
            if not self.road_elements:
                raise ValueError("clearance: the intersection has no road_elements, and no road was given")
            road = list(self.road_elements)
        return _flow_ids(self._push_mutations().clearance(first, count, road, d_event, events, per_sample), self.get_road_user_ids())

    def body_encounters(self, first=None, count=None, extents=None, gap_event=None, ttc_event=None, per_sample=True):
        """Engine.body_encounters on the population's own engine: the free gap and the time to contact between the road users'
        outlines over samples [first, first + count) of the engine's recording (step_n(..., dense=True) and advance_together record
        every tick in a ring of DENSE_CHUNK samples) or - first=None - now.  extents=None: every vehicle's own (vehicle_extents);
        else one (front, rear, half_width) for everybody or an [n, 3] array.  The result carries the partners also as the road
        users' ids: `ids`, gap_with_id, ttc_with_id [count, n] and run_gap_with_id, run_ttc_with_id [n] (None where there is no
        partner)."""
        if not self.vehicles:
            raise RuntimeError("the intersection is empty")
        if extents is None:
            extents = np.array([vehicle_extents(v) for v in self.vehicles], dtype=np.float64)
        return _body_ids(self._push_mutations().body_encounters(first, count, extents, gap_event, ttc_event, per_sample), self.get_road_user_ids())

    # ------------------------------------------------------------------ riders whose poles are drawn anew as their speed changes
    def _stochastic_riders(self):
        """the BalancingRiderBicycles with `stochastic_control_behavior=True` (parameters.py:1380-1396); cached until the population changes"""
        if self._stoch_for != len(self.vehicles) + self._stoch_epoch:
            self._stoch = [v for v in self.vehicles if getattr(v.params, "stochastic_control_behavior", False)]
            self._stoch_for = len(self.vehicles) + self._stoch_epoch
        return self._stoch

    def _resample_poles(self, riders, fx, fy):
        """BalancingRiderDynamics.step up to its gains (dynamics.py:617-647, 677-682), on the host, for the riders whose poles are
        drawn: the speed step (P controller, clamped acceleration, clamped speed - what the device is about to do with the same
        force), and where the speed changes `params.update_control_params((v_new + v) / 2)`, which draws new poles once the speed
        has moved 0.8333 m/s since the last draw.  In vehicle order: the draws come off one generator.  The tick is split for
        this - forces, draws, then the integration with the forces (csf_calc_forces / csf_apply_forces) - so that a rider steps
        with the poles the reference would have given it in THAT tick."""
        for r in riders:
            i, p, v_now = r._index, r.params, r._s[3]
            vd = np.sqrt(fx[i] ** 2 + fy[i] ** 2)
            a = min(max(p.k_p_v * (vd - v_now), p.a_max[0]), p.a_max[1])
            v_new = min(max(v_now + p.t_s * a, p.v_max_riding[0]), p.v_max_riding[1])
            if v_new != v_now:
                p.update_control_params((v_new + v_now) / 2)

    # ------------------------------------------------------------------ custom per-vehicle force hooks (vehicle.py:194-204, 250-299)
    def _field_engine(self, v):
        """an engine of the vehicle's class and parameter set, for its field alone (csf_pair_force: vehicle.py:1560-1648 /
        1054-1147 with THAT set's constants - the population's own engine evaluates set 0's)"""
        pod = v._pod(PRIORITY_RULES.get(self.priority_rule, 0))
        key = bytes(pod)
        eng = self._field_engines.get(key)
        if eng is None:
            eng = self._field_engines[key] = Engine(pod, 1)
        return eng

    def _hooked_forces(self, e):
        """calc_forces() of a population in which some vehicle carries a custom `rep_force_func` / `dest_force_func`
        (intersection.py:797-862, statement by statement): the hooks are the caller's Python, everything else comes from the
        engine's single-function entry points - csf_dest_force (queue pointer, navigation state, the class's destination force),
        csf_untracked (the mask), csf_pair_force (the class's field of one source at the receivers that track it) -, the column
        sum, the clamp and the road term are NumPy as in the reference.  O(n) device calls per tick: for the handful of road users
        scenarios with hooks have (the reference's own tick is slower still)."""
        from .utils import limitMagnitude

        n = self.n_bikes
        fdx, fdy = e.dest_force()                                  # :799 for every class force; advances the queues as the reference does
        self._pull(forces=False, advance=0)                        # vehicle.s / dest / destpointer as the hooks expect to find them
        X, Y, PSI = self._mirror.positions()
        for i, v in enumerate(self.vehicles):
            if v.dest_force_func is not None:                      # vehicle.py:295-297 (updateDestination has run: csf_dest_force)
                fdx[i], fdy[i] = v.dest_force_func(v)
        fx, fy = fdx.copy(), fdy.copy()
        if n > 1:
            U = e.untracked()                                      # [source, receiver], True: not considered (:690-745)
            Fx, Fy = np.zeros((n, n)), np.zeros((n, n))
            for i, v in enumerate(self.vehicles):
                trk = ~U[i]
                if not trk.any():
                    continue
                if v.rep_force_func is not None:                   # :814-820
                    fxi, fyi = v.rep_force_func(v, X[trk], Y[trk], PSI[trk])
                elif getattr(v.params, "f_0", 1.0) == 0.0 and v.MODEL != 0:
                    continue                                       # vehicle.py:1592-1593
                else:
                    fxi, fyi = self._field_engine(v).pair_force(v._s[:4].copy(), X[trk], Y[trk], PSI[trk])
                Fx[i, trk], Fy[i, trk] = fxi, fyi                  # :822-823
            frx, fry = limitMagnitude(Fx.sum(axis=0), Fy.sum(axis=0), np.sqrt(fdx ** 2 + fdy ** 2))   # :841-845
            fx, fy = frx + fdx, fry + fdy
        for el in self.road_elements:                              # :854-857
            fxe, fye = el.calcRepulsiveForce(X[:, None], Y[:, None])
            fx = fx + np.asarray(fxe).ravel()
            fy = fy + np.asarray(fye).ravel()
        return np.ascontiguousarray(fx, dtype=float), np.ascontiguousarray(fy, dtype=float)

    def step(self):
        """intersection.py:866-896: one simulation tick of the whole population."""
        if self.animate and self.is_first_step:          # intersection.py:881-885: everyone gets a drawing on the first tick
            for v in self.vehicles:
                if v.drawing is None:
                    v.add_drawing(self.ax, animated=True, **self.bicycle_drawing_kwargs)
        self.is_first_step = False
        why = self._host_reason()
        if why in (HOOKS, POLES):
            e = self._push_mutations()
            if self._hooked:
                fx, fy = self._hooked_forces(e)                    # intersection.py:889
            else:
                fx, fy = e.calc_forces()
            stochastic = self._stochastic_riders()
            if stochastic:
                self._resample_poles(stochastic, fx, fy)
                e = self._push_mutations()                         # (a new draw is a new parameter set of its rider)
            e.apply_forces(fx, fy)                                 # :891-892: every vehicle.step(Fx[i], Fy[i])
            self._pull(forces=True, advance=1)                     # :894
        elif why is None:
            self._push_mutations()
            self._pull(forces=True, advance=1, step=1)
        self.hist_n_vecs.append(self.n_bikes)

    def _host_reason(self, drawn=False, first_drawings=False):
        """Why every tick of this intersection has to pass the host, or None.  An empty intersection, custom force hooks and
        drawn poles bind every route; what a route cannot serve besides is its argument: `drawn` - the dense routes book a block
        of ticks afterwards, so no `animate`, no SUMO co-simulation, no drawing at all -, `first_drawings` - the batched route
        hands out no drawings, which `animate` wants on the first tick."""
        if self.n_bikes <= 0:
            return EMPTY
        if self._hooked:
            return HOOKS
        if self._stochastic_riders():
            return POLES
        if drawn and (self.animate or self.activate_sumo_cosimulation or any(v.drawing is not None for v in self.vehicles)):
            return DRAWN
        if first_drawings and self.animate and self.is_first_step:
            return FIRST_DRAWINGS
        return None

    def _dense_engine(self):
        """the engine, recording (Engine.record: it keeps the one-wave tick and the batched launch), when n ticks of this
        intersection can run in one call and be booked from the record afterwards; None when every tick has to pass the host
        (_host_reason) or the mirror's rows are wider than the engine's state"""
        if self._host_reason(drawn=True) is not None:
            return None
        e = self._push_mutations()
        if self._mirror.ns != e.ns:
            return None
        # A new engine gets its ring; the ring is sized for the engine's capacity and stays when road users come, go or are swapped
        # one for one: the engine itself begins a new stretch of the recording then (csf.h, "the lifetime of a recording"), and the
        # samples of the old roster are refused - to this intersection's encounters / post_encroachment / passing / flow as well.
        if not e._dense_ring:
            e.record(stride=1, capacity=DENSE_CHUNK, forces=True)
            e._dense_ring = True
        return e

    def step_n(self, n_ticks, pull=True, dense=False):
        """n_ticks ticks with no per-tick host work (the benchmark path).  `traj` receives only the final state, unless
        `dense`: then the engine records every tick on the device (Engine.record), the ticks run in calls as long as its ring,
        and vehicle.s, traj, trajF, F, znav, destpointer and hist_n_vecs are afterwards what n_ticks calls of step() leave."""
        if dense:
            left = int(n_ticks)
            while left > 0:
                e = self._dense_engine()
                if e is None:
                    self.step()
                    left -= 1
                    continue
                k = min(left, DENSE_CHUNK)
                tick = e.step_into(k, *self._mirror.live())
                self._book_block(*e.recorded(tick - k, k))
                left -= k
            return
        why = self._host_reason()
        if why in (HOOKS, POLES):                                     # (every tick passes the host)
            for _ in range(int(n_ticks)):
                self.step()
            return
        if why is None and n_ticks > 0:
            e = self._push_mutations()
            e.step(int(n_ticks))
            if pull:
                self._pull(forces=True, advance=int(n_ticks))
        self.hist_n_vecs.extend([self.n_bikes] * int(n_ticks))

    def _batch_outputs(self):
        """(engine, the bulk mirror's arrays for csf_step_batch_get_tick) when this intersection's tick can join a batched step,
        else None: _host_reason, or rows wider than the engine's state"""
        if self._host_reason(first_drawings=True) is not None:
            return None
        e = self._push_mutations()
        return (e, self._mirror.live()) if self._mirror.ns == e.ns else None

    def set_small_classes(self, on=True):
        """Engine.small_classes for this intersection's engine, now or when it is made: up to 32 road users with their own `params=`, of
        several vehicle classes or with UncontrolledVehicles among them take the one-wave tick - through step, step_n, step_together
        and advance_together (off by default)"""
        self._small_classes = bool(on)
        if self._engine is not None:
            self._engine.small_classes(self._small_classes)

    def set_mid_road(self, on=True):
        """Engine.mid_road for this intersection's engine, now or when it is made: 33 ... 2 175 road users between road edges of at most
        2 048 vertices take ONE launch per tick, road term included - through step, step_n, step_together and advance_together
        (off by default)"""
        self._mid_road = bool(on)
        if self._engine is not None:
            self._engine.mid_road(self._mid_road)

    def set_mid_classes(self, on=True):
        """Engine.mid_classes for this intersection's engine, now or when it is made: 33 ... 1 024 road users with their own `params=`,
        of several vehicle classes or with UncontrolledVehicles among them (no BalancingRiderBicycle) take ONE launch per tick - through
        step, step_n, step_together and advance_together (off by default)"""
        self._mid_classes = bool(on)
        if self._engine is not None:
            self._engine.mid_classes(self._mid_classes)

    def set_animated(self, animated):
        """intersection.py:899-915: switch every drawing between blitted (animated) and ordinary artists."""
        for v in self.vehicles:
            if v.drawing is not None and hasattr(v.drawing, "set_animated"):
                v.drawing.set_animated(animated)

    @property
    def engine(self):
        return self._engine_ready()


def _batch_of(engines):
    """the engines as ONE batch (Engine.batch_join), joined again when the set of engines changed - an intersection creates its
    engine lazily, or a new one when its population's vehicle classes change"""
    key = [id(e) for e in engines]
    if engines[0]._together is not None and [id(e) for e in engines[0]._together] == key:
        return
    for e in engines:
        old = e._together
        if old is None:
            continue
        try:
            Engine.batch_leave(old)
        except (_ffi.EngineError, ValueError):
            pass                                        # (a member was destroyed: the batch is gone already)
        for m in old:
            m._together = None
    Engine.batch_join(engines)
    for e in engines:
        e._together = list(engines)


def advance_together(intersections, n_ticks):
    """step_together(intersections, n_ticks) - the same vehicle.s, traj, trajF, F, znav, destpointer, hist_n_vecs - with the
    ticks in calls of up to DENSE_CHUNK: the engines record every tick on the device (Engine.record), a chunk is one
    csf_step_batch_get_tick (one launch per vehicle class) and one csf_batch_get_record (one gather, one transfer, one wait), and
    the host books the whole block at once (PopulationMirror.book_block) - instead of a call, a wait and the host's bookkeeping per tick.
    Intersections that need the host every tick (custom force hooks, stochastic riders, drawings or `animate`, SUMO
    co-simulation) and empty ones take step_together's route inside the same call."""
    intersections = list(intersections)
    left = int(n_ticks)
    while left > 0:
        k = min(left, DENSE_CHUNK)
        dense, rest = [], []
        for ins in intersections:
            e = ins._dense_engine()
            if e is None:
                rest.append(ins)
            else:
                dense.append((ins, e))
        if rest:
            step_together(rest, k)
        if dense:
            engines = [e for _, e in dense]
            _batch_of(engines)
            Engine.step_batch_into(engines, k, [ins._mirror.live() for ins, _ in dense])
            for (ins, _), (S, F, _) in zip(dense, Engine.batch_recorded(engines, k)):
                ins._book_block(S, F)
        left -= k


def _id_table(ids):
    """the table that turns a place in the population order into a road user's id"""
    return np.array(list(ids) + [None], dtype=object)             # (-1, no partner, takes the None at the end)


def _partner_ids(res, ids, fields):
    """a result with the road users' ids, and the partners of `fields` - places in the population order - also given as ids in
    <field>_id; returns the table"""
    names = _id_table(ids)
    res.ids = list(ids)
    for f in fields:
        setattr(res, f + "_id", None if getattr(res, f) is None else names[getattr(res, f)])
    return names


def _together(intersections, batch_call, add_ids, *args):
    """a measure over the last recorded samples of many intersections, all their engines in the same launches (batch_call: the
    Engine.batch_* of the measure, given the engines and args): a list with a result per intersection - add_ids has put the road
    users' ids into it -, None for an empty one and for one whose engine does not record"""
    intersections = list(intersections)
    live = [ins for ins in intersections if ins.vehicles]
    got = {}
    if live:
        engines = [ins._push_mutations() for ins in live]
        _batch_of(engines)
        for ins, res in zip(live, batch_call(engines, *args)):
            got[id(ins)] = None if res is None else add_ids(res, ins.get_road_user_ids())
    return [got.get(id(ins)) for ins in intersections]


def _encounter_ids(res, ids):
    """an Encounters with the partners' places in the population order also given as the road users' ids"""
    _partner_ids(res, ids, ("d_with", "ttc_with", "run_d_with", "run_ttc_with"))
    return res


def encounters_together(intersections, n_last, radius=0.5, d_event=None, ttc_event=None, per_sample=True):
    """SocialForceIntersection.encounters over the last n_last recorded samples of many intersections - those advance_together
    has just ticked - with all their engines in the same two launches, one transfer and one wait (Engine.batch_encounters): a list
    with a result per intersection, None for an empty one and for one whose engine does not record."""
    return _together(intersections, Engine.batch_encounters, _encounter_ids, n_last, radius, d_event, ttc_event, per_sample)


def _pet_ids(res, ids):
    """a PostEncroachment with the partners' places in the population order also given as the road users' ids"""
    names = _partner_ids(res, ids, ("seg_with", "run_with"))
    if res.events is not None:
        res.event_i_id, res.event_j_id = names[res.events["i"]], names[res.events["j"]]
    return res


def post_encroachment_together(intersections, n_last, pet_event=None, per_segment=True):
    """SocialForceIntersection.post_encroachment over the last n_last recorded samples of many intersections - those
    advance_together has just ticked - with all their engines in the same two launches, one transfer and one wait
    (Engine.batch_post_encroachment): a list with a result per intersection, None for an empty one and for one whose engine does
    not record."""
    return _together(intersections, Engine.batch_post_encroachment, _pet_ids, n_last, pet_event, per_segment)


def _passing_ids(res, ids):
    """a Passing with the partners' places in the population order also given as the road users' ids"""
    names = _partner_ids(res, ids, ("gap_with", "made_with", "by_with", "run_gap_with", "run_thw_with", "run_made_with", "run_by_with"))
    if res.events is not None:
        res.event_i_id, res.event_j_id = names[res.events["i"]], names[res.events["j"]]
    return res


def passing_together(intersections, n_last, band=0.75, lat_max=3.0, lat_event=None, per_station=True):
    """SocialForceIntersection.passing over the last n_last recorded samples of many intersections - those advance_together has
    just ticked - with all their engines in the same two launches, one transfer and one wait (Engine.batch_passing): a list with
    a result per intersection, None for an empty one and for one whose engine does not record."""
    return _together(intersections, Engine.batch_passing, _passing_ids, n_last, band, lat_max, lat_event, per_station)


def _flow_ids(res, ids):
    """a Flow with the road users' ids beside their places in the population order"""
    res.ids = list(ids)
    if res.events is not None:                                    # (no table without events: a batch has a thousand members)
        res.event_i_id = _id_table(ids)[res.events["i"]]
    return res


def flow_together(intersections, n_last, lines=None, areas=None, grid=None, events=False):
    """SocialForceIntersection.flow over the last n_last recorded samples of many intersections - those advance_together has
    just ticked - at one layout, with all their engines in the same two launches, one transfer and one wait (Engine.batch_flow):
    a list with a result per intersection, None for an empty one and for one whose engine does not record."""
    return _together(intersections, Engine.batch_flow, _flow_ids, n_last, lines, areas, grid, events)


def clearance_together(intersections, n_last, road, d_event=0.0, events=False, per_sample=True):
    """SocialForceIntersection.clearance over the last n_last recorded samples of many intersections - those advance_together has
    just ticked - at one road, with all their engines in the same three launches, one transfer and one wait
    (Engine.batch_clearance): a list with a result per intersection, None for an empty one and for one whose engine does not record."""
    return _together(intersections, Engine.batch_clearance, _flow_ids, n_last, road, d_event, events, per_sample)


def _body_ids(res, ids):
    """a BodyEncounters with the partners' places in the population order also given as the road users' ids"""
    _partner_ids(res, ids, ("gap_with", "ttc_with", "run_gap_with", "run_ttc_with"))
    return res


def body_encounters_together(intersections, n_last, extents=None, gap_event=None, ttc_event=None, per_sample=True):
    """SocialForceIntersection.body_encounters over the last n_last recorded samples of many intersections - those advance_together
    has just ticked - with all their engines in the same two launches, one transfer and one wait (Engine.batch_body_encounters).
    extents=None: every vehicle's own; else one (front, rear, half_width) for everybody or a list with an entry per intersection
    (None entries of empty ones are skipped).  A list with a result per intersection, None for an empty one and for one whose
    engine does not record."""
    intersections = list(intersections)
    live = [(k, ins) for k, ins in enumerate(intersections) if ins.vehicles]
    ext = extents
    if live and extents is None:
        ext = [np.array([vehicle_extents(v) for v in ins.vehicles], dtype=np.float64) for _, ins in live]
    elif live and not (hasattr(extents, "__len__") and len(extents) == 3 and all(np.isscalar(v) for v in extents)):
        if len(extents) != len(intersections):
            raise ValueError(f"body_encounters_together: {len(extents)} extents for {len(intersections)} intersections")
        ext = [extents[k] for k, _ in live]
    return _together(intersections, Engine.batch_body_encounters, _body_ids, n_last, ext, gap_event, ttc_event, per_sample)


def step_together(intersections, n_ticks=1):
    """Every SocialForceIntersection by n_ticks, exactly as `for ins in intersections: ins.step()` repeated n_ticks times would
    leave them - vehicle.s, traj, trajF, F, znav, hist_n_vecs, drawings, SUMO positions - with the ticks of all their engines in
    one csf_step_batch_get_tick per tick: the engines the one-wave tick takes run in one launch per vehicle class, and the host
    waits once.  Intersections with custom force hooks or stochastic riders take their own .step() (they pass the host every tick
    anyway); empty ones only count the tick.  The natural step_func of a Scenario over many junctions (SUMOScenario)."""
    intersections = list(intersections)
    for _ in range(int(n_ticks)):
        joined = []
        for ins in intersections:
            got = ins._batch_outputs()
            if got is None:
                ins.step()
            else:
                joined.append((ins, got[0], got[1]))
        if not joined:
            continue
        engines = [e for _, e, _ in joined]
        _batch_of(engines)
        Engine.step_batch_into(engines, 1, [o for _, _, o in joined])
        for ins, _, (_, _, _, fx, fy) in joined:
            ins.is_first_step = False
            ins._book_tick(fx, fy, True, 1)
            ins.hist_n_vecs.append(ins.n_bikes)

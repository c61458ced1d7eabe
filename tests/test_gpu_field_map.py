"""Force-field maps on the MI355X (include/csf.h: csf_field_map; csf_fieldmap.hip): the crowd's field and the road-edge term at
arbitrary probe points, against the CPU oracle and against the literal reference (tests/golden/field_map.npz, written by
tests/golden/make_golden_field_map.py).

Tolerances: the road term as tests/test_gpu_parity.py::test_road_force_exponent_paths_vs_oracle holds it - 5e-5 of
max(|F|, 1e-6) for probes at least 0.5 m from every vertex (an fp32 vertex offset resolves 4e-6 m, and r^-(sigma+1) amplifies that by
(sigma + 1) / r) -, the crowd term as test_calc_forces_golden holds column sums: rtol 2e-4, atol 2e-4 (Bicycle field: atol 2e-5 * 6,
test_gpu_parity.py:71).  The map does not depend on the pair kernel of the tick."""
import ctypes as C

import numpy as np
import pytest

from oracle import csf_oracle as orc
from conftest import mixed_classes

pytestmark = pytest.mark.gpu

CROWD_TOL = dict(rtol=2e-4, atol=2e-4)
BIKE_TOL = dict(rtol=2e-4, atol=2e-5 * 6.0)


@pytest.fixture(scope="module")
def amd():
    from cyclistsocialforce_amd import engine, parameters

    class NS:
        pass

    ns = NS()
    ns.Engine = engine.Engine
    ns.pod = parameters.default_pod
    return ns


def oparams(pod):
    return orc.Params.from_buffer_copy(bytes(pod))


def crowd_engine(amd, model, s0, rule=0, capacity=None, **over):
    s0 = np.asarray(s0, dtype=float)
    e = amd.Engine(amd.pod(model, priority_rule=rule, **over), capacity or max(len(s0), 1))
    e.add_agents(s0, 5.0)
    return e


def population(n, box, seed, with_queue=False):
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, 5))
    s0[:, 0], s0[:, 1] = rng.uniform(0, box, n), rng.uniform(0, box, n)
    s0[:, 2] = rng.uniform(-np.pi, np.pi, n)
    s0[:, 3] = rng.uniform(3, 6, n)
    if not with_queue:
        return s0
    d = np.array([50.0, 99.0, 100.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0], dq[:, 0, 1] = s0[:, 0], s0[:, 1]
    dq[:, 1:, 0] = s0[:, 0, None] + d[None, :] * np.cos(s0[:, 2])[:, None]
    dq[:, 1:, 1] = s0[:, 1, None] + d[None, :] * np.sin(s0[:, 2])[:, None]
    return s0, np.arange(n + 1) * 4, dq.reshape(-1, 3)


def masked_oracle(params, s, px, py, ppsi, cls=None, rule=0):
    """the unclamped, masked column sum a road user at every probe would get: the probe appended as the last road user"""
    n = s.shape[0]
    fx, fy = np.zeros(px.size), np.zeros(px.size)
    for k in range(px.size):
        x, y, psi, v = np.r_[s[:, 0], px[k]], np.r_[s[:, 1], py[k]], np.r_[s[:, 2], ppsi[k]], np.r_[s[:, 3], 0.0]
        if cls is None:
            a, b = orc.column_sums(params, x, y, psi, v, [n])
        else:
            a, b = orc.column_sums(params, x, y, psi, v, [n], cls=np.r_[cls, 0].astype(np.uint8), rule=rule)
        fx[k], fy[k] = a[0], b[0]
    return fx, fy


# ---- 1. road only, no road users ----------------------------------------------------------------------------------------------
def clear_probes(rng, verts, count, lo, hi):
    x, y = rng.uniform(lo[0], hi[0], 8 * count), rng.uniform(lo[1], hi[1], 8 * count)
    clear = np.min(np.hypot(x[:, None] - verts[None, :, 0], y[:, None] - verts[None, :, 1]), axis=1) >= 0.5
    assert clear.sum() >= count
    return x[clear][:count], y[clear][:count]


@pytest.mark.parametrize("sigmas", [(2.0, 2.0, 2.0), (3.0, 3.0, 3.0), (0.5, 4.0, 6.0)])
def test_road_only_vs_oracle(amd, sigmas):
    """intersection.py:226-242 summed over every vertex: the rsq-power path (one integer sigma) and the log2 / exp2 path, probe counts
    that end in a lane tail, a wave tail and a partial workgroup, one probe exactly on a vertex"""
    rng = np.random.default_rng(5)
    counts = (70, 64, 131)
    verts = np.vstack([np.c_[np.linspace(0, 40, c), 8.0 * k + rng.normal(0, 0.05, c)] for k, c in enumerate(counts)])
    off = np.r_[0, np.cumsum(counts)]
    F0, sg = np.array([0.15, 0.05, 0.3]), np.array(sigmas)
    X, Y = clear_probes(rng, verts, 257, (-5, -4), (45, 22))
    e = amd.Engine(amd.pod("planarpoint"), 1)
    e.set_road(off, verts, F0, sg)
    keep = np.ones(len(verts), bool); keep[10] = False
    v2 = verts[keep]; off2 = off.copy(); off2[1:] -= 1
    for m in (1, 63, 64, 65, 257):
        x, y = X[:m].copy(), Y[:m].copy()
        on = m // 2 if m > 1 else None
        if on is not None:
            x[on], y[on] = verts[10]                             # r = 0 for one vertex: that vertex adds nothing
        fx, fy = e.field_map(x, y, crowd=False, road=True)
        assert fx.shape == (m,) and np.isfinite(fx).all() and np.isfinite(fy).all()
        rx, ry = orc.road_forces(verts, off, F0, sg, x, y)
        scale = np.maximum(np.hypot(rx, ry), 1e-6)
        rest = np.arange(m) != (-1 if on is None else on)
        ex, ey = np.abs(fx - rx)[rest] / scale[rest], np.abs(fy - ry)[rest] / scale[rest]
        print(f"sigmas {sigmas} m {m}: road term off by {max(ex.max(), ey.max()):.2e} of max(|F|, 1e-6)")
        assert ex.max() < 5e-5 and ey.max() < 5e-5
        if on is not None:
            r0x, r0y = orc.road_force(v2, off2, F0, sg, x[on:on + 1], y[on:on + 1])
            assert abs(fx[on] - r0x[0]) < 2e-5 and abs(fy[on] - r0y[0]) < 2e-5


@pytest.mark.parametrize("sigma", [2.0, 2.5])
def test_road_two_vertex_tiles_far_from_the_origin(amd, sigma):
    """one edge of 1 100 vertices - two tiles of 1 024 - with the whole scene shifted by (5 000, -3 000) m: the probe's offset from a
    tile's origin is formed in fp64"""
    rng = np.random.default_rng(6)
    shift = np.array([5000.0, -3000.0])
    verts = np.c_[np.linspace(0, 110, 1100), rng.normal(0, 0.05, 1100)] + shift
    off, F0, sg = np.array([0, 1100]), np.array([0.15]), np.array([sigma])
    x, y = clear_probes(rng, verts, 65, shift + (-5, -6), shift + (115, 6))
    e = amd.Engine(amd.pod("planarpoint"), 1)
    e.set_road(off, verts, F0, sg)
    fx, fy = e.field_map(x, y, crowd=False, road=True)
    rx, ry = orc.road_forces(verts, off, F0, sg, x, y)
    scale = np.maximum(np.hypot(rx, ry), 1e-6)
    print(f"sigma {sigma}: road term off by {max((np.abs(fx - rx) / scale).max(), (np.abs(fy - ry) / scale).max()):.2e}")
    assert (np.abs(fx - rx) / scale).max() < 5e-5 and (np.abs(fy - ry) / scale).max() < 5e-5


# ---- 2. the curve scenario's road against the literal reference ---------------------------------------------------------------------
def curve_road():
    """scenarios/curve-scenario.py:63-81"""
    from cyclistsocialforce_amd import intersection as ci, parameters
    rp = parameters.RoadElementParameters(sigma=2.0, F_0=0.15)
    seg1 = ci.StraightRoadSegment(np.array((0, -20, np.pi / 2)), 5, 25, params=rp, ds=0.1)
    seg2 = ci.CurvedRoadSegment(seg1.x1, 5, 10, np.pi / 2, "right", params=rp, ds=0.1)
    seg3 = ci.CurvedRoadSegment(seg2.x1, 5, 10, np.pi / 2, "left", params=rp, ds=0.1)
    seg4 = ci.StraightRoadSegment(seg3.x1, 5, 20, params=rp, ds=0.1)
    return ci.RoadSegmentCollection((seg1, seg2, seg3, seg4))


def test_curve_road_vs_reference_fixture(golden):
    g = golden("field_map")
    X, Y = g["road_X"], g["road_Y"]
    road = curve_road()
    Fx, Fy = road.calcRepulsiveForce(X, Y)
    assert Fx.shape == X.shape and Fy.shape == X.shape
    verts = np.vstack([e.vertices for e in road.edges()])
    clear = np.min(np.hypot(X.ravel()[:, None] - verts[None, :, 0], Y.ravel()[:, None] - verts[None, :, 1]), axis=1).reshape(X.shape) >= 0.5
    assert clear.sum() > X.size // 2
    scale = np.maximum(np.hypot(g["road_Fx"], g["road_Fy"]), 1e-6)
    ex, ey = (np.abs(Fx - g["road_Fx"]) / scale)[clear], (np.abs(Fy - g["road_Fy"]) / scale)[clear]
    print(f"curve road: off by {max(ex.max(), ey.max()):.2e} of max(|F|, 1e-6) at {clear.sum()} probes")
    assert ex.max() < 5e-5 and ey.max() < 5e-5
    # the edges and the segments on their own add up to the collection (separate fp64 sums of fp32 terms: no bit equality asked)
    top = max(np.abs(Fx).max(), np.abs(Fy).max())
    for parts in (road.edges(), road.segs):
        sx, sy = np.zeros(X.shape), np.zeros(X.shape)
        for part in parts:
            px, py = part.calcRepulsiveForce(X, Y)
            assert px.shape == X.shape
            sx += px
            sy += py
        np.testing.assert_allclose(sx, Fx, rtol=1e-12, atol=1e-12 * top)
        np.testing.assert_allclose(sy, Fy, rtol=1e-12, atol=1e-12 * top)
    # the cache: new vertices, new engine
    edge = road.edges()[0]
    before = edge.calcRepulsiveForce(X[:1], Y[:1])[0].copy()
    edge.vertices = edge.vertices + np.array([0.5, 0.0])
    assert not np.array_equal(edge.calcRepulsiveForce(X[:1], Y[:1])[0], before)


# ---- 3. crowd, TwoD field, no mask ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 65])
def test_crowd_twod_vs_oracle(amd, n):
    s0 = population(n, 30.0, seed=n)
    rng = np.random.default_rng(100 + n)
    px, py, ppsi = rng.uniform(-5, 35, 130), rng.uniform(-5, 35, 130), rng.uniform(-np.pi, np.pi, 130)
    px[0], py[0] = s0[0, 0], s0[0, 1]                            # exactly on source 0: that source adds 0
    px[1], py[1] = s0[0, 0] + 3000.0, s0[0, 1]                   # 3 km away
    e = crowd_engine(amd, "twod", s0)
    fx, fy = e.field_map(px, py, ppsi, crowd=True, road=False)
    assert np.isfinite(fx).all() and np.isfinite(fy).all()
    P = orc.default_params("twod")
    rx, ry = np.zeros(130), np.zeros(130)
    for i in range(n):
        a, b = orc.pair_twod(P, s0[i, :3], px, py, ppsi)
        if i == 0:
            a[0] = b[0] = 0.0
        rx += a
        ry += b
    np.testing.assert_allclose(fx, rx, **CROWD_TOL)
    np.testing.assert_allclose(fy, ry, **CROWD_TOL)


def test_crowd_twod_vs_reference_fixture(amd, golden):
    g = golden("field_map")
    e = crowd_engine(amd, "twod", g["twod_s"])
    fx, fy = e.field_map(g["x"], g["y"], g["psi"], road=False)
    assert fx.shape == g["x"].shape
    np.testing.assert_allclose(fx, g["twod_Fx"], **CROWD_TOL)
    np.testing.assert_allclose(fy, g["twod_Fy"], **CROWD_TOL)


# ---- 4. crowd, Bicycle field ----------------------------------------------------------------------------------------------------------
def test_crowd_bicycle_vs_oracle_and_reference_fixture(amd, golden):
    s0 = population(3, 30.0, seed=44)
    s0[1, 3], s0[2, 3] = 0.0, 9.5                                # D3: v <= 0 -> e = 0; a fast one (e clamps at 0.7)
    rng = np.random.default_rng(45)
    px, py, ppsi = rng.uniform(-5, 35, 130), rng.uniform(-5, 35, 130), rng.uniform(-np.pi, np.pi, 130)
    e = crowd_engine(amd, "bicycle", s0)
    fx, fy = e.field_map(px, py, ppsi, road=False)
    P = orc.default_params("bicycle")
    rx, ry = np.zeros(130), np.zeros(130)
    for i in range(3):
        a, b = orc.pair_bicycle(P, s0[i, :3], s0[i, 3], px, py)
        rx += a
        ry += b
    np.testing.assert_allclose(fx, rx, **BIKE_TOL)
    np.testing.assert_allclose(fy, ry, **BIKE_TOL)
    g = golden("field_map")
    e2 = crowd_engine(amd, "bicycle", g["bicycle_s"])
    fx, fy = e2.field_map(g["x"], g["y"], g["psi"], road=False)
    np.testing.assert_allclose(fx, g["bicycle_Fx"], **BIKE_TOL)
    np.testing.assert_allclose(fy, g["bicycle_Fy"], **BIKE_TOL)


# ---- 5. mixed classes, own parameter sets, the mask -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
def test_mixed_classes_masked_vs_oracle(amd, golden, rule):
    g = golden("mixed")
    pods, cls = mixed_classes(g)
    s0 = g["s0"]
    n = s0.shape[0]
    e = amd.Engine(pods[0], n)
    e.set_param_classes(pods)
    e.add_agents(s0, g["vdes"])
    e.set_agent_class(np.arange(n), cls)
    e.set_priority_rule(rule)
    rng = np.random.default_rng(7 + rule)
    lo, hi = s0[:, :2].min(axis=0) - 5, s0[:, :2].max(axis=0) + 5
    px, py, ppsi = rng.uniform(lo[0], hi[0], 64), rng.uniform(lo[1], hi[1], 64), rng.uniform(-np.pi, np.pi, 64)
    fx, fy = e.field_map(px, py, ppsi, road=False, fov=True)
    rx, ry = masked_oracle([oparams(p) for p in pods], s0, px, py, ppsi, cls=cls, rule=rule)
    assert np.abs(rx).max() > 1e-2                              # (the probes feel the crowd)
    np.testing.assert_allclose(fx, rx, **CROWD_TOL)
    np.testing.assert_allclose(fy, ry, **CROWD_TOL)


# ---- 6. the mask is the reference's -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
def test_field_of_view_edges_decided_as_the_reference_decides(amd, rule):
    """probes whose source sits 1e-9 rad inside / outside an edge of their field of view, 4 m away: the force is non-zero exactly where
    get_untracked_foes tracks.  The two sources are 5.8 km apart - each adds exactly 0 at the other's probes (exp2 underflows)."""
    pod = amd.pod("twod", priority_rule=rule)
    hfov = pod.hfov
    src = np.array([[0.0, 0.0, 0.3, 5.0, 0.0], [5000.0, -3000.0, -2.0, 4.0, 0.0]])
    px, py, ppsi, want = [], [], [], []
    for s in src:
        for k, (edge, eps) in enumerate([(+1, 1e-9), (+1, -1e-9), (-1, 1e-9), (-1, -1e-9)]):
            psi = 0.4 + 0.7 * k + s[2]
            b = psi + edge * (0.5 * hfov + eps)                 # bearing of the source as the probe sees it
            x, y = s[0] - 4.0 * np.cos(b), s[1] - 4.0 * np.sin(b)
            U = orc.untracked_matrix(hfov, rule, [s[0], x], [s[1], y], [s[2], psi])
            px.append(x); py.append(y); ppsi.append(psi); want.append(not U[0, 1])
    px, py, ppsi, want = np.array(px), np.array(py), np.array(ppsi), np.array(want)
    if rule == 0:
        assert want.any() and not want.all()
    e = crowd_engine(amd, "twod", src, rule=rule)
    fx, fy = e.field_map(px, py, ppsi, road=False, fov=True)
    ux, uy = e.field_map(px, py, ppsi, road=False, fov=False)
    assert (np.hypot(ux, uy) > 1e-3).all()                      # (unmasked, every pair pushes)
    np.testing.assert_array_equal(np.hypot(fx, fy) > 0, want)
    np.testing.assert_array_equal(fx[want], ux[want])


def test_sign_of_phi_ahead_of_a_source_decided_as_the_reference_decides(amd):
    """probes straight ahead of a TwoD source, rotated by +-1e-9 rad off its heading line: np.sign(phi) (vehicle.py:1625) flips the
    tangential part, O(f_0) - a wrong decision cannot hide in the tolerance"""
    src = np.array([[0.0, 0.0, 0.3, 5.0, 0.0], [5000.0, -3000.0, -2.0, 4.0, 0.0]])
    px, py = [], []
    for s in src:
        for eps in (1e-9, -1e-9):
            px.append(s[0] + 4.0 * np.cos(s[2] + eps)); py.append(s[1] + 4.0 * np.sin(s[2] + eps))
    px, py, ppsi = np.array(px), np.array(py), np.full(4, 1.0)
    e = crowd_engine(amd, "twod", src)
    fx, fy = e.field_map(px, py, ppsi, road=False)
    P = orc.default_params("twod")
    rx, ry = np.zeros(4), np.zeros(4)
    for s in src:
        a, b = orc.pair_twod(P, s[:3], px, py, ppsi)
        rx += np.nan_to_num(a); ry += np.nan_to_num(b)
    assert np.abs(np.r_[rx[0] - rx[1], ry[0] - ry[1]]).max() > 0.5   # (the jump is there)
    np.testing.assert_allclose(fx, rx, **CROWD_TOL)
    np.testing.assert_allclose(fy, ry, **CROWD_TOL)


# ---- 7. skip / exclude ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", [0, 1])
def test_skip_gives_every_road_users_own_column_sum(amd, rule):
    s0 = population(16, 20.0, seed=16)
    e = crowd_engine(amd, "twod", s0, rule=rule)
    rx, ry = orc.column_sums(orc.default_params("twod", priority_rule=rule), s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3], np.arange(16))
    fx, fy = np.zeros(16), np.zeros(16)
    for j in range(16):
        a, b = e.field_map(s0[j, 0], s0[j, 1], s0[j, 2], road=False, fov=True, skip=j)
        assert a.shape == ()
        fx[j], fy[j] = a, b
    np.testing.assert_allclose(fx, rx, **CROWD_TOL)
    np.testing.assert_allclose(fy, ry, **CROWD_TOL)


def test_force_field_exclude_of_the_intersection(amd):
    from cyclistsocialforce_amd.intersection import SocialForceIntersection
    from cyclistsocialforce_amd.vehicle import TwoDBicycle
    s0 = population(16, 20.0, seed=16)
    vs = []
    for k, s in enumerate(s0):
        v = TwoDBicycle(tuple(s), id=f"v{k}")
        v.setDestinations(s[0] + np.array([30, 60]) * np.cos(s[2]), s[1] + np.array([30, 60]) * np.sin(s[2]))
        vs.append(v)
    ins = SocialForceIntersection(vs)
    rx, ry = orc.column_sums(orc.default_params("twod"), s0[:, 0], s0[:, 1], s0[:, 2], s0[:, 3], np.arange(16))
    for j in (0, 7, 15):
        a, b = ins.force_field(np.array([s0[j, 0]]), np.array([s0[j, 1]]), psi=s0[j, 2], road=False, fov=True, exclude=vs[j])
        np.testing.assert_allclose(a[0], rx[j], **CROWD_TOL)
        np.testing.assert_allclose(b[0], ry[j], **CROWD_TOL)
        a2, b2 = ins.force_field(np.array([s0[j, 0]]), np.array([s0[j, 1]]), psi=s0[j, 2], road=False, fov=True, exclude=f"v{j}")
        assert a2[0] == a[0] and b2[0] == b[0]
    with pytest.raises(ValueError):
        ins.force_field(np.zeros(2), np.zeros(2), exclude="nobody")
    vs[3].rep_force_func = lambda veh, x, y, psi: (0 * x, 0 * y)
    with pytest.raises(NotImplementedError):
        ins.force_field(np.zeros(2), np.zeros(2))


# ---- 8. determinism -------------------------------------------------------------------------------------------------------------------
def road_and_crowd(amd):
    rng = np.random.default_rng(8)
    s0 = population(40, 30.0, seed=8)
    verts = np.c_[np.linspace(-5, 35, 300), -6.0 + rng.normal(0, 0.05, 300)]
    e = crowd_engine(amd, "twod", s0, rule=1)
    e.set_road(np.array([0, 300]), verts, np.array([0.15]), np.array([2.0]))
    px, py, ppsi = rng.uniform(-5, 35, 257), rng.uniform(-5, 35, 257), rng.uniform(-np.pi, np.pi, 257)
    return e, px, py, ppsi


def test_a_probes_bits_do_not_depend_on_the_call(amd, monkeypatch):
    monkeypatch.setenv("CSF_PAIR_VARIANT", "0")
    e, px, py, ppsi = road_and_crowd(amd)
    n0 = e.field_map_launches()
    fx, fy = e.field_map(px, py, ppsi, crowd=True, road=True, fov=True)
    assert e.field_map_launches() == n0 + 2                     # one launch per term, whatever m is
    gx, gy = e.field_map(px, py, ppsi, crowd=True, road=True, fov=True)
    assert e.field_map_launches() == n0 + 4
    assert np.array_equal(fx, gx) and np.array_equal(fy, gy)
    for k in range(257):                                         # every probe alone
        a, b = e.field_map(px[k:k + 1], py[k:k + 1], ppsi[k:k + 1], crowd=True, road=True, fov=True)
        assert a[0] == fx[k] and b[0] == fy[k], k
    n1 = e.field_map_launches()
    cx, cy = e.field_map(px, py, ppsi, crowd=True, road=False, fov=True)
    assert e.field_map_launches() == n1 + 1
    qx, qy = e.field_map(px, py, crowd=False, road=True)
    assert e.field_map_launches() == n1 + 2
    assert np.array_equal(cx + qx, fx) and np.array_equal(cy + qy, fy)   # crowd + road, added in fp64, the crowd term first
    monkeypatch.setenv("CSF_PAIR_VARIANT", "1")
    e1, _, _, _ = road_and_crowd(amd)
    hx, hy = e1.field_map(px, py, ppsi, crowd=True, road=True, fov=True)
    assert np.array_equal(fx, hx) and np.array_equal(fy, hy)


# ---- 9. the simulation is not disturbed, the state is current ---------------------------------------------------------------------------
@pytest.mark.auto_variant
@pytest.mark.parametrize("n", [3, 200, 4096])
def test_map_between_steps_leaves_the_run_alone_and_reads_the_current_state(amd, n):
    """the engine's own tick for the size - one wave, one launch, pair + per-agent launches side by side -: step(5), map, step(5) ends
    bit for bit where step(10) of a twin ends, and the map after step(5) is the oracle's on e.state() of that tick"""
    box = max(20.0, 3.0 * np.sqrt(n))
    s0, off, dq = population(n, box, seed=n, with_queue=True)
    engines = []
    for _ in range(2):
        e = crowd_engine(amd, "twod", s0)
        e.set_dest_queue(np.arange(n), off, dq, reset=True)
        engines.append(e)
    a, b = engines
    rng = np.random.default_rng(9)
    px, py, ppsi = rng.uniform(0, box, 24), rng.uniform(0, box, 24), rng.uniform(-np.pi, np.pi, 24)
    a.step(5)
    fx, fy = a.field_map(px, py, ppsi, road=False, fov=True)
    st = a.state()
    a.step(5)
    b.step(10)
    assert np.array_equal(a.state(), b.state())
    fa, fb = a.forces(), b.forces()
    assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1])
    rx, ry = masked_oracle(orc.default_params("twod"), st, px, py, ppsi)
    np.testing.assert_allclose(fx, rx, **CROWD_TOL)
    np.testing.assert_allclose(fy, ry, **CROWD_TOL)


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_have_a_message_and_no_side_effect(amd):
    from calib_common import data_set, pod_sets
    s0, off, dq = population(40, 30.0, seed=10, with_queue=True)
    engines = []
    for _ in range(2):
        e = crowd_engine(amd, "twod", s0)
        e.set_dest_queue(np.arange(40), off, dq, reset=True)
        engines.append(e)
    a, twin = engines
    lib = a._lib
    m = 5
    x, y, psi, fx, fy = (np.zeros(m) for _ in range(5))
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)              # noqa: E731
    X, Y, PSI, FX, FY = p(x), p(y), p(psi), p(fx), p(fy)
    cases = {
        "x NULL": (m, None, Y, PSI, 3, -1, FX, FY), "y NULL": (m, X, None, PSI, 3, -1, FX, FY),
        "Fx NULL": (m, X, Y, PSI, 3, -1, None, FY), "Fy NULL": (m, X, Y, PSI, 3, -1, FX, None),
        "psi NULL with CROWD": (m, X, Y, None, 1, -1, FX, FY), "m < 0": (-1, X, Y, PSI, 3, -1, FX, FY),
        "what 0": (m, X, Y, PSI, 0, -1, FX, FY), "unknown bit": (m, X, Y, PSI, 8 | 1, -1, FX, FY),
        "FOV without CROWD": (m, X, Y, PSI, 4 | 2, -1, FX, FY), "skip too large": (m, X, Y, PSI, 1, 40, FX, FY),
        "skip below -1": (m, X, Y, PSI, 1, -2, FX, FY),
    }
    n0 = a.field_map_launches()
    for name, args in cases.items():
        rc = lib.csf_field_map(a._h, *args)
        assert rc in (-1, -4), (name, rc)
        assert lib.csf_last_error(a._h).decode(), name
    assert a.field_map_launches() == n0 and (fx == 0).all() and (fy == 0).all()
    assert lib.csf_field_map(a._h, 0, None, None, None, 3, -1, None, None) == 0   # m == 0 is fine and writes nothing
    # psi may be NULL without the crowd term
    assert lib.csf_field_map(a._h, m, X, Y, None, 2, -1, FX, FY) == 0 and (fx == 0).all()   # (no road: zeros)
    a.step(5); twin.step(5)
    assert np.array_equal(a.state(), twin.state())
    # an empty population gives zeros; non-finite probes give NaN for that probe only
    empty = amd.Engine(amd.pod("twod"), 4)
    zx, zy = empty.field_map(np.ones(3), np.ones(3), 0.0, crowd=True, road=True)
    assert (zx == 0).all() and (zy == 0).all()
    bx, by = a.field_map(np.array([1.0, np.nan, 2.0, np.inf]), np.array([1.0, 1.0, np.inf, 2.0]), np.array([0.0, 0.0, 0.0, 0.0]), road=False)
    assert np.isfinite(bx[0]) and np.isnan(bx[1:]).all() and np.isnan(by[1:]).all()
    # a member of a loopback group
    g = [crowd_engine(amd, "twod", s0) for _ in range(2)]
    amd.Engine.loopback_group(g)
    rc = lib.csf_field_map(g[0]._h, m, X, Y, PSI, 1, -1, FX, FY)
    assert rc == -4 and lib.csf_last_error(g[0]._h).decode()
    # an engine that holds a calibration data set
    sets = pod_sets("twod", 2)
    cs0, cFx, cFy = data_set("twod", n_seq=2, ticks=20)
    c = amd.Engine(sets[0], 4)
    c.calib_load(cs0, cFx, cFy, np.zeros((20, 2, 2)), [0, 1], max_sets=2)
    rc = lib.csf_field_map(c._h, m, X, Y, PSI, 1, -1, FX, FY)
    assert rc == -4 and lib.csf_last_error(c._h).decode()

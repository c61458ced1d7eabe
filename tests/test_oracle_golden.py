"""Pins the CPU oracle (oracle/csf_oracle.c) to the golden vectors captured from the literal reference.

Every case cites the reference function it pins.  Tolerances: 1e-12 relative where the oracle follows
the same arithmetic; 2e-7 on single calls where the reference itself goes through an iterative solver (MINPACK lm,
dynamics.py:1070) or FITPACK (vehicle.py:1496-1510).  Measured: population trajectories agree with the
literal reference to <= 1.1e-11 absolute over 150-3100 ticks (1e-9 asserted).
"""
import numpy as np
import pytest

from oracle import csf_oracle as orc


def test_limit_angle_and_angle_difference(golden):
    g = golden("utils")
    got = np.array([orc.limit_angle(t) for t in g["a"]])
    np.testing.assert_allclose(got, g["limitAngle"], rtol=0, atol=1e-15)         # utils.py:124-139
    got = np.array([orc.angle_difference(p, q) for p, q in zip(g["a1"], g["a2"])])
    np.testing.assert_allclose(got, g["angleDifference"], rtol=0, atol=1e-15)    # utils.py:151-182
    lx, ly = orc.limit_magnitude(g["x"], g["y"], g["r"])
    np.testing.assert_allclose(lx, g["lx"], rtol=1e-15)                          # utils.py:56-86
    np.testing.assert_allclose(ly, g["ly"], rtol=1e-15)


def test_pair_field_twod(golden):
    """vehicle.py:1560-1648 (TwoDBicycle.calcRepulsiveForce)."""
    g = golden("pair_fields")
    p = orc.default_params("twod")
    fx = np.zeros(g["x"].size); fy = np.zeros(g["x"].size)
    for k in range(g["x"].size):
        a, b = orc.pair_twod(p, g["src"][k], g["x"][k:k + 1], g["y"][k:k + 1], g["psi"][k:k + 1])
        fx[k], fy[k] = a[0], b[0]
    scale = np.hypot(g["twod_fx"], g["twod_fy"])
    np.testing.assert_allclose(fx, g["twod_fx"], rtol=1e-11, atol=1e-13 * scale.max())
    np.testing.assert_allclose(fy, g["twod_fy"], rtol=1e-11, atol=1e-13 * scale.max())
    # survey known answers
    np.testing.assert_allclose(fx[:4], [1.4335766673611808e-01, -5.5699677693686585e-03,
                                        -3.6663914817607920e-03, 6.3346542039922857e+00], rtol=1e-12)


def test_pair_field_bicycle(golden):
    """vehicle.py:1054-1147 (Bicycle.calcRepulsiveForce / calcPotential / updateExcentricity)."""
    g = golden("pair_fields")
    p = orc.default_params("bicycle")
    fx = np.zeros(g["x"].size); fy = np.zeros(g["x"].size)
    for k in range(g["x"].size):
        a, b = orc.pair_bicycle(p, g["src"][k], g["src_v"][k], g["x"][k:k + 1], g["y"][k:k + 1])
        fx[k], fy[k] = a[0], b[0]
    np.testing.assert_allclose(fx, g["bicycle_fx"], rtol=1e-11, atol=1e-14)
    np.testing.assert_allclose(fy, g["bicycle_fy"], rtol=1e-11, atol=1e-14)


def test_pair_field_guard_far_apart():
    """Deviation D1: where the reference underflows to 0/0 the oracle returns exactly 0 (SURVEY finding 4)."""
    p = orc.default_params("twod")
    fx, fy = orc.pair_twod(p, (0.0, 0.0, 0.0), np.array([-3000.0, 0.0]), np.array([8000.0, 0.0]),
                           np.array([0.0, 0.3]))
    assert fx[0] == 0.0 and fy[0] == 0.0          # underflow
    assert fx[1] == 0.0 and fy[1] == 0.0          # coincident (D2)
    assert np.isfinite(fx).all() and np.isfinite(fy).all()


@pytest.mark.parametrize("tag", ["n2", "n3", "n16", "n32", "n16_p2r"])
def test_untracked_masks_and_totals(golden, tag):
    """intersection.py:690-745 (get_untracked_foes) and 747-864 (calc_forces)."""
    g = golden("masks_totals")
    rule = int(g[f"{tag}_p2r"])
    p = orc.default_params("twod", priority_rule=rule)
    s0 = g[f"{tag}_s0"]
    U = orc.untracked_matrix(p.hfov, rule, s0[:, 0], s0[:, 1], s0[:, 2])
    np.testing.assert_array_equal(U, g[f"{tag}_untracked0"])
    pop = orc.Population(p, s0, g[f"{tag}_vdes"], g[f"{tag}_off"], g[f"{tag}_dq"])
    pop.step(1)
    s1 = pop.state()
    np.testing.assert_allclose(s1, g[f"{tag}_s1"], rtol=1e-11, atol=1e-12)
    U1 = orc.untracked_matrix(p.hfov, rule, s1[:, 0], s1[:, 1], s1[:, 2])
    np.testing.assert_array_equal(U1, g[f"{tag}_untracked1"])
    pop.calc_forces_range(0, pop.n)
    fx, fy = pop.forces()
    np.testing.assert_allclose(fx, g[f"{tag}_Fx1"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(fy, g[f"{tag}_Fy1"], rtol=1e-7, atol=1e-9)


def test_control_move(golden):
    """vehicle.py:1218-1272 (Bicycle.control + Bicycle.move) incl. the survey's known answer."""
    g = golden("control_move")
    for k in range(g["s"].shape[0]):
        p = orc.default_params("bicycle" if g["is_bicycle"][k] else "twod")
        out = orc.control_move(p, g["s"][k], np.r_[g["dest"][k, :2], 0.0], g["dest"][k, 2] != 0,
                               g["F"][k, 0], g["F"][k, 1])
        np.testing.assert_allclose(out, g["s_next"][k], rtol=1e-12, atol=1e-13, err_msg=f"case {k}")
    np.testing.assert_allclose(g["s_next"][0], [1.0378922590640614, 2.011843424463476, 0.3029352011084877,
                                                3.97, 0.07380026035475676], rtol=1e-14)


@pytest.mark.parametrize("tag", ["demo_a", "turn", "stop_last", "stop_mid", "pp_turn"])
def test_dest_force_runs(golden, tag):
    """vehicle.py:354-457, 545-594, 1416-1558: single agent driven by its own destination force."""
    g = golden("dest_force_runs")
    model = str(g[f"{tag}_model"])
    p = orc.default_params(model)
    S = g[f"{tag}_s"]
    dq = g[f"{tag}_dq"]
    pop = orc.Population(p, S[:1], float(g[f"{tag}_vdes"]), np.array([0, dq.shape[0]]), dq)
    T = g[f"{tag}_Fdest"].shape[0]
    tol = 2e-7
    for t in range(T):
        fx, fy = pop.dest_force(0)
        ptr, zn, i, st = pop.nav()
        assert st[0] == 0
        np.testing.assert_allclose([fx, fy], g[f"{tag}_Fdest"][t], rtol=tol, atol=tol, err_msg=f"tick {t}")
        assert ptr[0] == g[f"{tag}_ptr"][t], f"tick {t}"
        np.testing.assert_array_equal(zn[0], g[f"{tag}_znav"][t], err_msg=f"tick {t}")
        pop.apply_forces([fx], [fy])
        np.testing.assert_allclose(pop.state()[0], S[t + 1], rtol=tol, atol=tol, err_msg=f"tick {t}")


def test_planarpoint_steps(golden):
    """dynamics.py:996-1079 (closed-form implicit midpoint vs the reference's lm solve)."""
    g = golden("planarpoint_steps")
    p = orc.default_params("planarpoint")
    for k in range(g["s01"].shape[0]):
        s0 = g["s01"][k, :4]
        pop = orc.Population(p, s0[None, :], 5.0, np.array([0, 1]), np.array([[s0[0], s0[1], 0.0]]))
        pop.apply_forces([g["F01"][k, 0]], [g["F01"][k, 1]])
        np.testing.assert_allclose(pop.state()[0], g["s01"][k, 4:], rtol=1e-7, atol=1e-8)
        pop.apply_forces([g["F01"][k, 2]], [g["F01"][k, 3]])
        np.testing.assert_allclose(pop.state()[0], g["s2"][k], rtol=1e-7, atol=1e-8)


def test_road_edges(golden):
    """intersection.py:118-242 on the scenarios/curve-scenario.py:63-81 geometry."""
    g = golden("road_edges")
    fx, fy = orc.road_force(g["verts"], g["off"], g["F0"], g["sigma"], g["x"], g["y"])
    np.testing.assert_allclose(fx, g["Fx"], rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(fy, g["Fy"], rtol=1e-11, atol=1e-13)


def test_expm_against_scipy():
    from scipy.linalg import expm
    rng = np.random.default_rng(0)
    for scale in (0.01, 1.0, 30.0, 400.0):
        A = rng.normal(size=(6, 6)) * scale / 6
        A -= np.eye(6) * scale * 0.5
        np.testing.assert_allclose(orc.expm(A), expm(A), rtol=1e-9, atol=1e-12)


TRAJ = [
    # (prefix, model, rule, rtol on positions) — intersection.py:866-896 end to end
    ("demo_twod", "twod", 0, 1e-9), ("demo_bicycle", "bicycle", 0, 1e-9),
    ("demo_planarpoint", "planarpoint", 0, 1e-9), ("demo_invpend", "invpend", 0, 1e-9),
    ("dense_twod", "twod", 0, 1e-9), ("dense_bicycle", "bicycle", 0, 1e-9),
    ("dense_planarpoint", "planarpoint", 0, 1e-9), ("dense_invpend", "invpend", 0, 1e-9),
    ("p2r_twod", "twod", 1, 1e-9), ("road_pp", "planarpoint", 0, 1e-9), ("lap_twod", "twod", 0, 1e-9),
]


@pytest.mark.parametrize("prefix,model,rule,tol", TRAJ)
def test_population_trajectories(golden, prefix, model, rule, tol):
    g = golden("trajectories")
    p = orc.default_params(model, priority_rule=rule)
    pop = orc.Population(p, g[f"{prefix}_s0"], g[f"{prefix}_vdes"], g[f"{prefix}_off"], g[f"{prefix}_dq"])
    if f"{prefix}_verts" in g.files:
        pop.set_road(g[f"{prefix}_roff"], g[f"{prefix}_verts"], g[f"{prefix}_F0"], g[f"{prefix}_sigma"])
    S = g[f"{prefix}_S"]
    F = g[f"{prefix}_F"]
    every = {"lap_twod": 50}.get(prefix, 10)
    for k in range(1, S.shape[0]):
        pop.step(every)
        got = pop.state()
        np.testing.assert_allclose(got, S[k], rtol=tol, atol=tol * 10, err_msg=f"{prefix} sample {k}")
        fx, fy = pop.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=100 * tol, atol=100 * tol,
                                   err_msg=f"{prefix} forces sample {k}")
    assert (pop.nav()[3] == 0).all()


def test_invpend_yaw_step_without_control_shim(golden):
    """A11 pinned independently of the `control` stand-in: the scenario of the reference's own test
    (src/cyclistsocialforce/test.py:15-165: 30 deg yaw step, 10 s, speed held at v_desired_default) on the reference's
    closed-loop matrices, integrated by scipy.signal.cont2discrete('zoh') and by scipy's Radau ODE solver
    (tests/golden/make_golden.py: gen_invpend_yawstep).  The oracle's step (vehicle.py:1810-1848) must follow it."""
    g = golden("invpend_yawstep")
    assert np.abs(g["ode"] - g["zoh"]).max() < 1e-12 and np.abs(g["shim"] - g["zoh"]).max() < 1e-12
    v = float(g["v"])
    p = orc.default_params("invpend")
    pop = orc.Population(p, np.array([[0.0, 0, 0, v, 0, 0]]), v, [0, 1], [[0.0, 0.0, 0.0]])
    T = g["Fx"].size
    got = np.zeros((T, 3))
    for k in range(T):
        pop.apply_forces(g["Fx"][k:k + 1], g["Fy"][k:k + 1])
        s = pop.state()[0]
        assert abs(s[3] - v) < 1e-12                      # |F| = v_desired: the speed loop holds the speed
        got[k] = (s[2], s[4], s[5])
    np.testing.assert_allclose(got, g["zoh"], rtol=1e-7, atol=1e-11)     # the reference test's own rtol (test.py:100-118)
    # test.py's expected curve comes from pole placement whose gains are the predecessor of HEAD's table
    # (parameters.py:1858-1861 vs 1863-1883): recorded, not asserted equal
    np.testing.assert_allclose(g["K_place_testpy"], [6.26092881, -48.635, -6.92845026, -2.25215286, -2.15918001], rtol=1e-7)
    assert abs(g["K_table_head"][0] - g["K_place_testpy"][0]) > 100


def test_planarbike_against_reference(golden):
    """PlanarBicycle (vehicle.py:2031-2076; dynamics.py:178-258, 1167-1226): gains re-derived from the
    speed every step, single steps, the 3-bike demo geometry (700 ticks) and a dense population (150 ticks), all captured
    from the reference (tests/golden/make_golden.py: gen_planarbike)."""
    g = golden("planarbike")
    p = orc.default_params("planarbike")
    s01, F = g["steps_s01"], g["steps_F01"]
    for k in range(0, s01.shape[0], 7):
        kx, ku = orc.planarbike_gains(p, s01[k, 3])
        np.testing.assert_allclose(np.r_[kx, ku], g["steps_gains"][k], rtol=1e-10)
    n = s01.shape[0]
    pop = orc.Population(p, s01[:, :5], 5.0, np.arange(n + 1), np.c_[s01[:, 0], s01[:, 1], np.zeros(n)])
    pop.apply_forces(F[:, 0], F[:, 1])
    np.testing.assert_allclose(pop.state(), s01[:, 5:], rtol=1e-12, atol=1e-12)
    pop.apply_forces(F[:, 2], F[:, 3])
    np.testing.assert_allclose(pop.state(), g["steps_s2"], rtol=1e-12, atol=1e-12)
    for tag in ("demo", "dense"):
        pop = orc.Population(p, g[f"{tag}_s0"], g[f"{tag}_vdes"], g[f"{tag}_off"], g[f"{tag}_dq"])
        S = g[f"{tag}_S"]
        for k in range(1, S.shape[0]):
            pop.step(10)
            np.testing.assert_allclose(pop.state(), S[k], rtol=0, atol=1e-9, err_msg=f"{tag} sample {k}")
        np.testing.assert_allclose(np.c_[pop.forces()], g[f"{tag}_F"][-1], rtol=0, atol=1e-8)


@pytest.mark.parametrize("model,tol", [("twod", 1e-9), ("bicycle", 1e-9), ("invpend", 1e-9)])
def test_population_with_individual_parameter_sets(golden, model, tol):
    """Every reference vehicle owns its params object (vehicle.py:64-204): the field of vehicle i is evaluated with ITS
    f_0 / sigma / e (vehicle.py:1592-1612; p_0 / p_decay for the Bicycle field), masked with ITS hfov
    (intersection.py:733-735), and it steers, accelerates and arrives with its own limits and gains.  Four parameter sets
    dealt round-robin over 10-16 vehicles, trajectories captured from the literal reference (make_golden.py: gen_hetero)."""
    from conftest import hetero_classes

    g = golden("hetero")
    pods, cls = hetero_classes(g, model)
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in pods]
    pop = orc.Population(classes[0], g[f"{model}_s0"], g[f"{model}_vdes"], g[f"{model}_off"], g[f"{model}_dq"])
    pop.set_classes(classes, cls)
    S, F = g[f"{model}_S"], g[f"{model}_F"]
    for k in range(1, S.shape[0]):
        pop.step(10)
        np.testing.assert_allclose(pop.state(), S[k], rtol=tol, atol=tol * 10, err_msg=f"{model} sample {k}")
        fx, fy = pop.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=100 * tol, atol=100 * tol, err_msg=f"{model} forces {k}")
    # and the uniform oracle on the same start does NOT follow it: the parameter sets matter
    uni = orc.Population(classes[0], g[f"{model}_s0"], g[f"{model}_vdes"], g[f"{model}_off"], g[f"{model}_dq"])
    uni.step(10 * (S.shape[0] - 1))
    assert np.abs(uni.state()[:, :2] - S[-1][:, :2]).max() > 1e-2


def test_population_of_several_vehicle_classes(golden):
    """intersection.py:797-823 calls each vehicle's own calcDestinationForce / calcRepulsiveForce / step: Bicycle,
    TwoDBicycle, InvPendulumBicycle, PlanarPointBicycle and PlanarBicycle in ONE intersection (three of each, the third with
    parameters of its own), 250 ticks captured from the literal reference (make_golden.py: gen_mixed)."""
    from conftest import mixed_classes

    g = golden("mixed")
    pods, cls = mixed_classes(g)
    classes = [orc.Params.from_buffer_copy(bytes(p)) for p in pods]
    pop = orc.Population(classes[0], g["s0"], g["vdes"], g["off"], g["dq"], ns=6)
    pop.set_classes(classes, cls)
    S, F = g["S"], g["F"]
    for k in range(1, S.shape[0]):
        pop.step(10)
        np.testing.assert_allclose(pop.state(), S[k], rtol=1e-9, atol=1e-8, err_msg=f"sample {k}")
        fx, fy = pop.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=1e-7, atol=1e-7, err_msg=f"forces {k}")


def test_uncontrolled_vehicle_among_cyclists_golden(golden):
    """UncontrolledVehicle (vehicle.py:920-988) in one intersection with cyclists, as the reference ran it
    (tests/golden/uncontrolled.npz): a car that follows its prescribed trajectory (and stays where it ends), one without
    a trajectory (it reads the zeros of the ring it was constructed with: the origin from its first tick on); both exert
    the TwoDBicycle field with their CarParameters and feel nothing."""
    g = golden("uncontrolled")
    n = g["s0"].shape[0]
    tab = [orc.default_params("twod"), orc.default_params("uncontrolled"),
           orc.default_params("uncontrolled", hfov=float(g["parked_hfov"]), f_0=float(g["parked_f0"]))]
    cls = np.array([0] * (n - 2) + [1, 2], dtype=np.uint8)
    pop = orc.Population(tab[0], g["s0"], g["vdes"], g["off"], g["dq"], ns=6)
    pop.set_classes(tab, cls)
    pop.set_script(g["script_off"], g["script_rows"])
    S, F = g["S"], g["F"]
    for k in range(1, S.shape[0]):
        pop.step(10)
        np.testing.assert_allclose(pop.state(), S[k], rtol=0, atol=1e-9, err_msg=f"sample {k}")
        fx, fy = pop.forces()
        np.testing.assert_allclose(np.c_[fx, fy], F[k - 1], rtol=0, atol=1e-9, err_msg=f"forces of sample {k}")
    assert np.array_equal(S[-1, -1], np.zeros(6)) and abs(S[-1, -2, 1] - (-7.0 + 5.0 * 1.79)) < 1e-12


# ------------------------------------------------------------------ BalancingRiderBicycle
def test_whipple_carvallo_matrices_against_the_paper(golden):
    """The canonical matrices of the linearised Whipple-Carvallo bicycle (parameters.py:1284-1300 takes them from
    bicycleparameters, which is absent here): the formulas of Meijaard, Papadopoulos, Ruina & Schwab (2007), Appendix A, against
    the paper's own benchmark - M, C1, K0, K2 of its table-1 bicycle and the eigenvalues of its table 2, typed in from the paper
    (tests/golden/make_golden_balancingrider.py)."""
    g = golden("balancingrider")
    bench = dict(zip([str(k) for k in g["wc_benchmark_names"]], [float(v) for v in g["wc_benchmark_params"]]))
    M, C1, K0, K2 = orc.whipple_carvallo(bench)
    for got, name in ((M, "M"), (C1, "C1"), (K0, "K0"), (K2, "K2")):
        np.testing.assert_allclose(got, g[f"wc_benchmark_{name}"], rtol=0, atol=2e-13, err_msg=name)
    Minv = np.linalg.inv(M)
    for v, want in zip(g["wc_benchmark_eig_v"], g["wc_benchmark_eig"]):
        A = np.zeros((4, 4))
        A[0:2, 2:4] = np.eye(2)
        A[2:4, 0:2] = -Minv @ (bench["g"] * K0 + v * v * K2)
        A[2:4, 2:4] = -Minv @ (v * C1)
        np.testing.assert_allclose(np.sort_complex(np.linalg.eigvals(A)), want, rtol=0, atol=2e-12, err_msg=f"v = {v}")


def test_balancingrider_pole_functions_against_the_reference_polemodel(golden):
    """parameters.py:1352-1411 -> controlbehavior.py PoleModel.get_component_mean_function: the straight lines over speed that
    give a rider's desired poles, computed by the host package's restatement (polemodel.py) from the reference's model files
    (their copies under tests/golden/balancingriderparams), and its tabulated copy of them, against what the reference's own
    PoleModel returned (make_golden_balancingrider.py executes the reference's controlbehavior.py)."""
    import os

    from cyclistsocialforce_amd import polemodel as pm

    g = golden("balancingrider")
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "balancingriderparams")
    for tag in ("BR0", "BR1"):
        name = f"{tag}_ImRe5GivenV_pole-model-params.yaml"
        np.testing.assert_allclose(pm.MEAN_FUNCTIONS[name], g[f"polefun_{tag}"], rtol=0, atol=1e-13)
        np.testing.assert_allclose(pm.component_mean_functions(os.path.join(here, name)), g[f"polefun_{tag}"], rtol=0, atol=1e-13)
        for v, want in zip(g[f"poles_{tag}_v"], g[f"poles_{tag}"]):
            np.testing.assert_allclose(pm.poles_at(pm.MEAN_FUNCTIONS[name][0], v), want, rtol=0, atol=1e-12)


def test_balancingrider_gains_and_steps_against_the_reference(golden):
    """dynamics.py:600-615 (pole placement per speed: the reference calls control.place = scipy.signal.place_poles under the
    golden script's shim; the oracle uses Ackermann's formula - one input, one solution) and :664-705 (the implicit midpoint
    step, which the reference solves with MINPACK and the oracle as the linear system it is): gains at six speeds, and one
    vehicle on 120 prescribed forces, state for state."""
    g = golden("balancingrider")
    P = orc.default_params("balancingrider")
    for v, K in zip(g["gains_v"], g["gains"]):
        np.testing.assert_allclose(orc.balancingrider_gains(P, v), K, rtol=1e-11, atol=1e-12, err_msg=f"v = {v}")
    S, F = g["steps_S"], g["steps_F"]
    pop = orc.Population(P, S[:1], 5.0, np.array([0, 1]), np.array([[S[0, 0], S[0, 1], 0.0]]))
    for t in range(F.shape[0]):
        pop.apply_forces(F[t:t + 1, 0], F[t:t + 1, 1])
        np.testing.assert_allclose(pop.state()[0], S[t + 1], rtol=0, atol=1e-10, err_msg=f"step {t}")


@pytest.mark.parametrize("tag", ["demo", "dense", "stddemo"])
def test_balancingrider_population_trajectories(golden, tag):
    """three and sixteen BalancingRiderBicycles through the literal SocialForceIntersection.step (TwoD field, direct-approach
    destination force, vehicle.py:1953-1990): 300 / 200 ticks, every tenth state; stddemo: the reference's DEFAULT demo,
    demoCSFstandalone.py -m balancingrider, 700 ticks"""
    g = golden("balancingrider")
    pop = orc.Population(orc.default_params("balancingrider"), g[f"{tag}_s0"], g[f"{tag}_vdes"], g[f"{tag}_off"], g[f"{tag}_dq"])
    S = g[f"{tag}_S"]
    for k in range(1, S.shape[0]):
        pop.step(10)
        np.testing.assert_allclose(pop.state(), S[k], rtol=0, atol=1e-9, err_msg=f"sample {k}")


def test_balancingrider_between_road_edges(golden):
    """three riders on the road of scenarios/curve-scenario.py through the literal SocialForceIntersection.step with road_elements
    (intersection.py:226-242, 853-857): 300 ticks, every tenth state"""
    g = golden("balancingrider")
    pop = orc.Population(orc.default_params("balancingrider"), g["road_s0"], g["road_vdes"], g["road_off"], g["road_dq"])
    pop.set_road(g["road_roff"], g["road_verts"], g["road_F0"], g["road_sigma"])
    S = g["road_S"]
    for k in range(1, S.shape[0]):
        pop.step(10)
        np.testing.assert_allclose(pop.state(), S[k], rtol=0, atol=1e-9, err_msg=f"sample {k}")

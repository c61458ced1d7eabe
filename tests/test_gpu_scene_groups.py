"""Rider groups with candidate parameter sets of their own in a closed-loop calibration: csf_scene_calib_groups and
csf_scene_calib_eval_groups against twin engines on the general path that hold per-vehicle parameter sets, against the oracle, against
the evaluation without groups, with the other hooks, the refusals and the optimiser."""
import functools

import numpy as np
import pytest

from scene_calib_common import VDES, field_sets
from scene_groups_common import (ACT_SCENES, ACT_TICKS, G, GENERAL_TOL, GROUP, GROUPS, LENGTHS, MODELS, N_RIDERS, ORACLE_GROUP, ORACLE_TICKS, R,
                                 ROFF, T, act_pods, act_scene, general_twin, group_scenes, group_sets, oracle_case, oracle_group_run)
from test_gpu_scene_calib import _check_sums, _sums_reference

pytestmark = [pytest.mark.gpu, pytest.mark.auto_variant]

FEAT = np.array([0, 2, 4, 5], dtype=np.int32)   # x, psi, delta, theta: rows 4 / 5 lie beyond n_states of some classes


def _engine(pod, cap):
    from cyclistsocialforce_amd.engine import Engine
    return Engine(pod, cap)


@functools.lru_cache(maxsize=None)
def _job(model):
    s0, off, rows, per = group_scenes(model)
    obj = np.random.default_rng(1).normal(size=(T, R, len(FEAT)))
    return dict(sets=group_sets(model), s0=s0, off=off, rows=rows, per=per, obj=obj)


def _loaded(job, groups=True, n_riders=N_RIDERS, lengths=LENGTHS, max_sets=3):
    e = _engine(job["sets"][0][0], max_sets * int(np.sum(n_riders)))
    e.scene_calib_load(n_riders, job["s0"], VDES, job["off"], job["rows"], job["obj"], FEAT, lengths=lengths, max_sets=max_sets)
    if groups:
        e.scene_calib_groups(GROUP, G)
    return e


def _against_twins(model, states, sets, per, groups, lengths, roff, what, **hooks):
    """every (candidate, scene) of `states` against its general-path twin: all state rows of the riders the twin has, at every tick"""
    n_all, worst = int(roff[-1]), 0.0
    for k, pods in enumerate(sets):
        for q, (sq, oq, dq) in enumerate(per):
            ln = int(lengths[q])
            if ln == 0:
                continue
            kw = {name: val[q] for name, val in hooks.items()}
            tw = general_twin(pods, groups[q], sq, oq, dq, ln, **kw)
            got = states[:ln, k * n_all + roff[q]: k * n_all + roff[q + 1]]
            there = np.isfinite(tw[..., 0])
            assert np.isfinite(got[there]).all(), (k, q)
            d = float(np.abs(got[there] - tw[there]).max()) if there.any() else 0.0
            worst = max(worst, d)
            assert d < GENERAL_TOL, (what, model, k, q, d)
    print(f"{model} {what}: largest |scene_calib_eval_groups - general-path twin| over all state rows and ticks = {worst:.3e} (bound {GENERAL_TOL:g})")
    return worst


@pytest.mark.parametrize("model", MODELS)
def test_grouped_scenes_against_general_path_twins(model):
    """Six scenes (2, 5, 32, 3, 1, 4 riders; lengths 40, 25, 40, 40, 40, 0; groups: one of each / mixed / round robin over four / all
    in group 0 / the rider in group 1 / three groups, empty) x 3 candidates of 4 parameter sets - different field, field of view, gains and
    v_max_riding per group, one candidate with the second priority rule, one with it in group 1's record alone - in one launch, the states
    after every tick against a twin engine per (candidate, scene) on the general path that holds the four sets as parameter classes.
    Bound: 2e-5 on every state row, what tests/test_gpu_small.py holds between the one-wave tick and the general path after 300
    ticks.  The sums are NumPy's on the returned states within 2 m 2^-53; the same call twice and a permuted order of candidates give
    the same rows."""
    job = _job(model)
    sets = job["sets"]
    e = _loaded(job)
    before = e.scene_calib_launches()
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    assert e.scene_calib_launches() == before + 1
    assert states.shape == (T, 3 * R, e.ns) and sums.shape == (3, R, 2)
    _against_twins(model, states, sets, job["per"], GROUPS, LENGTHS, ROFF, "scenes")
    w = _check_sums(sums, _sums_reference(states, job["obj"], FEAT, LENGTHS, ROFF, 3), LENGTHS, ROFF, len(FEAT))
    print(f"{model}: sums at {w:.3f} of the bound 2 m 2^-53")
    # an ended scene keeps its last state, an empty one its start
    q = 1
    assert np.array_equal(states[LENGTHS[q]:, ROFF[q]: ROFF[q + 1]], np.tile(states[LENGTHS[q] - 1, ROFF[q]: ROFF[q + 1]], (T - LENGTHS[q], 1, 1)))
    assert np.all(sums[:, ROFF[5]: ROFF[6]] == 0.0)
    sums2, states2 = e.scene_calib_eval_groups(sets, states=True)
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2)
    perm = [2, 0, 1]
    sums3, states3 = e.scene_calib_eval_groups([sets[k] for k in perm], states=True)
    for at, k in enumerate(perm):
        assert np.array_equal(sums3[at], sums[k]) and np.array_equal(states3[:, at * R: (at + 1) * R], states[:, k * R: (k + 1) * R])
    e.close()


def test_three_riders_in_group_0_with_two_groups_loaded():
    """the scene of 3 riders alone, everybody in group 0, n_groups = 2 loaded: group 1's record is nobody's, and the evaluation is the
    general-path twin's (2e-5) and, within the same bound, scene_calib_eval's of group 0's sets on a never-grouped engine (another
    kernel instance: equal to rounding)"""
    job = _job("twod")
    sq, oq, dq = job["per"][3]
    sets = [p[:2] for p in job["sets"]]
    obj = job["obj"][:, :3]
    e = _engine(sets[0][0], 9)
    e.scene_calib_load([3], sq, VDES, oq, dq, obj, FEAT, max_sets=3)
    e.scene_calib_groups(np.zeros(3, dtype=np.uint8), 2)
    sums, states = e.scene_calib_eval_groups(sets, states=True)
    _against_twins("twod", states, sets, [(sq, oq, dq)], [np.zeros(3, dtype=int)], [T], np.array([0, 3]), "3 riders in group 0 of 2")
    e.close()
    plain = _engine(sets[0][0], 9)
    plain.scene_calib_load([3], sq, VDES, oq, dq, obj, FEAT, max_sets=3)
    s0, st0 = plain.scene_calib_eval([p[0] for p in sets], states=True)
    diff = float(np.abs(states - st0).max())
    print(f"3 riders in group 0 of 2 against the ungrouped evaluation: {diff:.3e}")
    assert diff < GENERAL_TOL
    plain.close()


@pytest.mark.parametrize("rule", [0, 1])
def test_grouped_scene_against_the_oracle(rule):
    """TwoD, 5 riders in two groups, 200 free ticks, 3 candidates whose groups differ in the field, the field of view and v_max_riding:
    positions after every 10th tick within 1e-4 x extent of orc.Population with set_classes - the bound of the oracle case of
    tests/test_gpu_scene_replay.py; tests/test_scene_groups_host.py holds the oracle's own sensitivity to 1e-7 m at the start below
    1e-5 x extent on this case"""
    s0, off, dq, pods = oracle_case(rule)
    e = _engine(pods[0][0], 3 * 5)
    e.scene_calib_load([5], s0, VDES, off, dq, np.zeros((ORACLE_TICKS, 5, 2)), [0, 1], max_sets=3)
    e.scene_calib_groups(ORACLE_GROUP, 2)
    _, states = e.scene_calib_eval_groups(pods, states=True, stride=10)
    worst = 0.0
    for k, pd in enumerate(pods):
        ref = oracle_group_run(pd, ORACLE_GROUP, s0, off, dq)
        ext = max(np.ptp(ref[..., 0]), np.ptp(ref[..., 1]), 14.0)
        got = states[:, k * 5: (k + 1) * 5, :2]
        dev = float(np.hypot(got[..., 0] - ref[..., 0], got[..., 1] - ref[..., 1]).max()) / ext
        worst = max(worst, dev)
        assert dev < 1e-4, (rule, k, dev)
    print(f"rule {rule}: largest |scene_calib_eval_groups - oracle| = {worst:.2e} x extent")
    e.close()


@pytest.mark.parametrize("model", MODELS)
def test_no_groups_means_today(model):
    """after scene_calib_groups(None), and with n_groups == 1, scene_calib_eval_groups with 1-tuples gives array_equal sums and states to
    scene_calib_eval on an engine that never had groups"""
    job = _job(model)
    ones = [p[:1] for p in job["sets"]]
    plain = _loaded(job, groups=False)
    s0, st0 = plain.scene_calib_eval([p[0] for p in ones], states=True)
    s1, st1 = plain.scene_calib_eval_groups(ones, states=True)       # (no groups loaded: n_groups == 1)
    assert np.array_equal(s0, s1) and np.array_equal(st0, st1)
    plain.close()
    e = _loaded(job)
    e.scene_calib_eval_groups(job["sets"])
    e.scene_calib_groups(None)
    s2, st2 = e.scene_calib_eval(list(p[0] for p in ones), states=True)
    s3, st3 = e.scene_calib_eval_groups(ones, states=True)
    assert np.array_equal(s0, s2) and np.array_equal(st0, st2) and np.array_equal(s0, s3) and np.array_equal(st0, st3)
    e.scene_calib_groups(GROUP, 1)                                    # (n_groups <= 1 drops them as well)
    s4, st4 = e.scene_calib_eval([p[0] for p in ones], states=True)
    assert np.array_equal(s0, s4) and np.array_equal(st0, st4)
    e.close()


@pytest.mark.parametrize("model", MODELS)
def test_labels_are_only_labels(model):
    """swapping the labels 0 and 1 in `group` together with the two records of every candidate gives array_equal results: the sources
    of a receiver are summed in rider order whatever their group (csf_small_body.inc: the constants are looked up per source)"""
    job = _job(model)
    e = _loaded(job)
    s0, st0 = e.scene_calib_eval_groups(job["sets"], states=True)
    swapped = GROUP.copy()
    swapped[GROUP == 0], swapped[GROUP == 1] = 1, 0
    e.scene_calib_groups(swapped, G)
    s1, st1 = e.scene_calib_eval_groups([(p[1], p[0], p[2], p[3]) for p in job["sets"][:2]], states=True)
    # (candidates 0 and 1: every record has the candidate's priority rule.  The last candidate's rule is its FIRST record's, which the swap
    # would change.)
    assert np.array_equal(s0[:2], s1) and np.array_equal(st0[:, : 2 * R], st1)
    e.close()


def test_the_groups_act_and_identical_groups_are_no_groups():
    """on the two seeded TwoD scenes (scene_groups_common.ACT_SCENES) every rider differs from the run where group 1 carries group 0's
    set; a candidate whose groups carry identical parameters agrees with the ungrouped evaluation of that set within the tolerance of
    the twin test (2e-5).  The order of every sum is kept, but the grouped kernel is a compilation of its own of the per-agent tick, and
    the compiler contracts a few of its fp64 chains differently: equal to rounding, not bit for bit."""
    base, other = act_pods()
    for k in range(len(ACT_SCENES)):
        s0, off, dq, grp = act_scene(k)
        n = s0.shape[0]
        e = _engine(base, 2 * n)
        e.scene_calib_load([n], s0, VDES, off, dq, np.zeros((ACT_TICKS, n, 2)), [0, 1], max_sets=2)
        _, plain = e.scene_calib_eval([base, other], states=True)
        e.scene_calib_groups(grp, 2)
        _, st = e.scene_calib_eval_groups([(base, base), (base, other), (other, other)][:2], states=True)
        same, act = st[:, :n], st[:, n:]
        diff = float(np.abs(same - plain[:, :n]).max())
        print(f"acting scene {k}: identical groups against the ungrouped evaluation: {diff:.3e}")
        assert diff < GENERAL_TOL
        moved = np.abs(act[..., :2] - same[..., :2]).max(axis=(0, 2))
        print(f"acting scene {k}: every rider moved by at least {moved.min():.2e} m")
        assert np.all(moved > 1e-6), (k, moved)
        _, st2 = e.scene_calib_eval_groups([(other, other)], states=True)
        assert float(np.abs(st2 - plain[:, n:]).max()) < GENERAL_TOL
        e.close()


def _hook_job(model):
    """scenes 0 - 2 of the data set (2, 5, 32 riders; 40, 25, 40 ticks) for the tests with the other hooks"""
    job = _job(model)
    nr, ln = N_RIDERS[:3], LENGTHS[:3]
    n = int(nr.sum())
    return dict(job, s0=job["s0"][:n], off=job["off"][: n + 1], rows=job["rows"][: job["off"][n]], per=job["per"][:3], obj=job["obj"][:, :n]), nr, ln, n


@pytest.mark.parametrize("model", MODELS)
def test_groups_with_replay(model):
    """groups + replay: rider 1 of the scene of 2 (group 1), riders 1 and 4 of the scene of 5 (group 1) and every third of the 32 follow
    a recording made with another candidate; against the general-path twin that pushes the recording after every tick (2e-5); rows 0 - 3
    of the replayed riders ARE the recording, their sums exactly (0, 0); twice and permuted: array_equal"""
    job, nr, ln, n = _hook_job(model)
    roff = np.r_[0, np.cumsum(nr)]
    sets = job["sets"]
    masks = [np.array([False, True]), np.array([False, True, False, False, True]), np.arange(32) % 3 == 0]
    mask = np.concatenate(masks)
    e = _loaded(job, groups=False, n_riders=nr, lengths=ln)
    e.scene_calib_groups(GROUP[:n], G)
    _, rec = e.scene_calib_eval_groups(sets[2:3], states=True)       # the recording: candidate 2, nobody replayed
    assert np.isfinite(rec).all()
    e.scene_calib_replay(mask, rec[:, mask, :4])
    sums, states = e.scene_calib_eval_groups(sets[:2], states=True)
    recs = [rec[:, roff[q]: roff[q + 1]] for q in range(3)]
    _against_twins(model, states, sets[:2], job["per"], GROUPS[:3], ln, roff, "replay", replayed=masks, rec=recs)
    for k in range(2):
        for q in range(3):
            got = states[: ln[q], k * n + roff[q]: k * n + roff[q + 1]]
            assert np.array_equal(got[:, masks[q], :4], recs[q][: ln[q]][:, masks[q], :4]), (k, q)
    assert np.all(sums[:, mask] == 0.0) and np.all(sums[:, ~mask] > 0.0)
    sums2, states2 = e.scene_calib_eval_groups(sets[:2], states=True)
    sums3, states3 = e.scene_calib_eval_groups([sets[1], sets[0]], states=True)
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2)
    assert np.array_equal(sums3[0], sums[1]) and np.array_equal(sums3[1], sums[0]) and np.array_equal(states3[:, :n], states[:, n:])
    e.close()


@pytest.mark.parametrize("model", MODELS)
def test_groups_with_presence_windows(model):
    """groups + presence windows: riders enter late and leave early in the scenes of 5 and of 32; against the general-path twin whose
    riders join by add_agents + set_agent_class and leave by remove_agents (2e-5 on the present cells)"""
    job, nr, ln, n = _hook_job(model)
    roff = np.r_[0, np.cumsum(nr)]
    enter = [np.array([0, 0]), np.array([0, 3, 0, 10, 0]), np.zeros(32, dtype=int)]
    exit_ = [np.array([40, 40]), np.array([25, 25, 18, 25, 25]), np.full(32, 40)]
    enter[2][1::4] = 2 + 4 * np.arange(8)
    exit_[2][2::4] = 12 + 3 * np.arange(8)
    e = _loaded(job, groups=False, n_riders=nr, lengths=ln)
    e.scene_calib_groups(GROUP[:n], G)
    e.scene_calib_windows(np.concatenate(enter).astype(np.int32), np.concatenate(exit_).astype(np.int32))
    sums, states = e.scene_calib_eval_groups(job["sets"], states=True)
    _against_twins(model, states, job["sets"], job["per"], GROUPS[:3], ln, roff, "windows", enter=enter, exit=exit_)
    sums2, states2 = e.scene_calib_eval_groups(job["sets"], states=True)
    sums3, _ = e.scene_calib_eval_groups(job["sets"][::-1], states=True)
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2) and np.array_equal(sums3[::-1], sums)
    e.close()


@pytest.mark.parametrize("model", MODELS)
def test_groups_with_road_edges_and_road_parameters_per_candidate(model):
    """groups + road edges with road_F_0 per candidate: two polylines beside the box of every scene, F_0 and sigma of all vertices replaced
    per candidate (an integer sigma and a fractional one); against the general-path twin with that road set by set_road (2e-5)"""
    job, nr, ln, n = _hook_job(model)
    roff = np.r_[0, np.cumsum(nr)]
    from scene_road_common import box_of
    f0s, sgs = np.array([0.4, 0.9, 0.2]), np.array([2.0, 3.0, 2.5])
    es, off, vs, roads = [], [0], [], []
    for q in range(3):
        box = box_of(model, int(nr[q]))
        lines = [np.c_[np.linspace(-20.0, box + 20.0, c), np.full(c, y)] for c, y in ((40, -3.0), (23, box + 3.0))]
        for v in lines:
            es.append(q), vs.append(v), off.append(off[-1] + len(v))
        roads.append((np.array([0, 40, 63], dtype=np.int64), np.concatenate(lines)))
    e = _loaded(job, groups=False, n_riders=nr, lengths=ln)
    e.scene_calib_groups(GROUP[:n], G)
    e.scene_calib_road(np.array(es, dtype=np.int32), np.array(off, dtype=np.int64), np.concatenate(vs), 0.3, 2.0)
    sums, states = e.scene_calib_eval_groups(job["sets"], road_F0=f0s, road_sigma=sgs, states=True)
    worst = 0.0
    for k, pods in enumerate(job["sets"]):
        for q, (sq, oq, dq) in enumerate(job["per"]):
            road = (roads[q][0], roads[q][1], np.full(2, f0s[k]), np.full(2, sgs[k]))
            tw = general_twin(pods, GROUPS[q], sq, oq, dq, int(ln[q]), road=road)
            got = states[: ln[q], k * n + roff[q]: k * n + roff[q + 1]]
            d = float(np.abs(got - tw).max())
            worst = max(worst, d)
            assert d < GENERAL_TOL, (model, k, q, d)
    print(f"{model} road: largest |scene_calib_eval_groups - general-path twin| = {worst:.3e} (bound {GENERAL_TOL:g})")
    sums2, states2 = e.scene_calib_eval_groups(job["sets"], road_F0=f0s, road_sigma=sgs, states=True)
    sums3 = e.scene_calib_eval_groups(job["sets"][::-1], road_F0=f0s[::-1], road_sigma=sgs[::-1])
    assert np.array_equal(sums, sums2) and np.array_equal(states, states2) and np.array_equal(sums3[::-1], sums)
    e.close()


def test_refusals_leave_the_engine_as_it_was():
    from cyclistsocialforce_amd._ffi import EngineError
    from cyclistsocialforce_amd import parameters
    job = _job("twod")
    sets = job["sets"]
    e = _loaded(job)
    s0, st0 = e.scene_calib_eval_groups(sets, states=True)
    bad = GROUP.copy()
    bad[7] = 4
    for call in (lambda: e.scene_calib_groups(GROUP, 5),                                     # n_groups 5
                 lambda: e.scene_calib_groups(bad, 4),                                       # an entry out of range
                 lambda: e.scene_calib_groups(np.minimum(GROUP, 1) * 3, 3),                  # ... also below the limit of 4
                 lambda: e.scene_calib_eval_groups([p[:2] for p in sets]),                   # a wrong n_groups at eval
                 lambda: e.scene_calib_eval_groups([p[:3] + (parameters.default_pod("bicycle"),) for p in sets]),   # a record of another class
                 lambda: e.scene_calib_eval([p[0] for p in sets]),                           # plain eval while groups are loaded
                 lambda: e.scene_calib_eval([p[0] for p in sets], road_F0=1.0, road_sigma=2.0)):
        with pytest.raises(EngineError) as err:
            call()
        assert len(str(err.value)) > 20
        s1, st1 = e.scene_calib_eval_groups(sets, states=True)
        assert np.array_equal(s0, s1) and np.array_equal(st0, st1)
    # the hostile calls of the raw C ABI (tests/hostile_caller.py has the list for the older entry points): a negative code, a message,
    # and the same evaluation afterwards
    import ctypes as C
    from cyclistsocialforce_amd import _ffi
    L, h = e._lib, e._h
    tab = (_ffi.Params * (3 * G))(*[p for t in sets for p in t])
    out = np.zeros((3, R, 2))
    po = out.ctypes.data_as(C.c_void_p)
    size, abi = C.sizeof(_ffi.Params), _ffi.ABI_VERSION
    hostile = [lambda: L.csf_scene_calib_eval_groups(h, 3, G, tab, size - 8, abi, None, None, po, 1, None),      # another csf_params
               lambda: L.csf_scene_calib_eval_groups(h, 3, G, tab, size, abi + 1, None, None, po, 1, None),      # another ABI
               lambda: L.csf_scene_calib_eval_groups(h, 3, G, None, size, abi, None, None, po, 1, None),         # no records
               lambda: L.csf_scene_calib_eval_groups(h, 3, G, tab, size, abi, None, None, None, 1, None),        # nowhere to put the sums
               lambda: L.csf_scene_calib_eval_groups(h, 0, G, tab, size, abi, None, None, po, 1, None),          # no candidate
               lambda: L.csf_scene_calib_eval_groups(h, 4, G, tab, size, abi, None, None, po, 1, None),          # more than max_sets
               lambda: L.csf_scene_calib_eval_groups(h, 3, G, tab, size, abi, None, None, po, 0, None),          # stride 0
               lambda: L.csf_scene_calib_eval_groups(h, 3, 0, tab, size, abi, None, None, po, 1, None),          # no group
               lambda: L.csf_scene_calib_eval_groups(h, 3, -1, tab, size, abi, None, None, po, 1, None),
               lambda: L.csf_scene_calib_eval_groups(h, 3, G, tab, size, abi, po, None, po, 1, None),            # road_F0 without road_sigma
               lambda: L.csf_scene_calib_groups(h, GROUP.ctypes.data_as(C.c_void_p), 1 << 30)]
    for k, call in enumerate(hostile):
        rc = call()
        assert rc < 0 and len(L.csf_last_error(h)) > 20, (k, rc)
        s1, st1 = e.scene_calib_eval_groups(sets, states=True)
        assert np.array_equal(s0, s1) and np.array_equal(st0, st1), k
    assert L.csf_scene_calib_groups(None, None, 2) == -1 and L.csf_scene_calib_eval_groups(None, 1, 1, None, 0, 0, None, None, None, 1, None) == -1
    e.close()
    # a shared and a wide load refuse groups and evaluate as before
    sq, oq, dq = job["per"][1]
    for wide in (False, True):
        x = _engine(sets[0][0], 15)
        load = x.scene_calib_load_wide if wide else x.scene_calib_load_shared
        load([5], [5], np.arange(5), np.zeros(5, dtype=int), np.full(5, 25), sq, VDES, oq, dq, job["obj"][:25, :5], FEAT, max_sets=3,
             **(dict(wide_from=1) if wide else {}))
        a = x.scene_calib_eval([p[0] for p in sets])
        with pytest.raises(EngineError) as err:
            x.scene_calib_groups(GROUPS[1], 2)
        assert "lanes" in str(err.value)
        assert np.array_equal(a, x.scene_calib_eval([p[0] for p in sets]))
        x.close()
    # no data set
    x = _engine(sets[0][0], 4)
    with pytest.raises(EngineError):
        x.scene_calib_groups(np.zeros(4, dtype=np.uint8), 2)
    x.close()


def test_two_groups_f_0_are_recovered_from_leave_one_out_scenes():
    """TwoD, two groups with true f_0 of 1.0 x and 1.6 x the default: 12 leave-one-out scenes (ego_split of three recorded scenes of 4
    riders, 60 ticks), fitting (("f_0", 0), ("f_0", 1)) from a guess 20 % off with the settings of the recovery of DESIGN.md 4.10: xtol
    1e-4, maxiter 400, ftol 1e-30; theta within xtol of theta*, the objective below 1e-6 of its start value"""
    from cyclistsocialforce_amd import calibration as cal, parameters, vehicle
    from scene_calib_common import crowd
    base = parameters.default_pod("twod")
    true = np.array([base.f_0, 1.6 * base.f_0])
    grp = np.array([0, 1, 0, 1], dtype=np.uint8)
    data = []
    for seed in (1230, 1222, 1224):     # (chosen with the CPU oracle: either f_0 moves at least three of the four riders by centimetres)
        x, y, psi, v, off, dq = crowd(4, seed=seed, box=8.0)
        s0 = np.c_[x, y, psi, v, np.zeros(4)]
        e = _engine(base, 4)
        e.scene_calib_load([4], s0, VDES, off, dq, np.zeros((60, 4, 2)), [0, 1], max_sets=1)
        e.scene_calib_groups(grp, 2)
        _, traj = e.scene_calib_eval_groups([(parameters.default_pod("twod", f_0=true[0]), parameters.default_pod("twod", f_0=true[1]))], states=True)
        e.close()
        data += cal.SceneData(s0, VDES, off, dq, traj[:, :, :4], group=grp).ego_split()
    assert len(data) == 12
    c = cal.InteractionCalibration(vehicle.TwoDBicycle, [("f_0", 0), ("f_0", 1)], data, data, [1, 1, 0, 0, 0, 0], group_params=[{}, {}],
                                   max_sets=8, maxiter=400, xtol=1e-4, ftol=1e-30)
    guess = true * np.array([1.2, 0.8])
    f_start = float(c.evaluate([guess])[0])
    res = c.run(guess)
    print(f"recovered f_0 = {res[0]} (true {true}), objective {res[1]:.3e} from {f_start:.3e}, {res[2]} iterations")
    assert res[1] < 1e-6 * f_start
    assert np.abs(res[0] - true).max() < 1e-4
    c.close()

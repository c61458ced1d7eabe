"""The default side-by-side path (CSF_CHASE=1) as a fresh process meets it (run as a script in a process of its own by
tests/test_gpu_chase.py::test_the_default_path_in_a_fresh_process, one model per process).

Which order an engine of the headline kind takes is decided once per process (tick.inc: chase_take, g_chase_found): by the first
engine's own measurement, which starts at the first re-binning at or after tick 256 of a call long enough for three periods - a
step(600) from tick 0, or bench.py's scratch pre-roll - with some 250 ticks still queued on the main stream.  Later engines take the
decision over.  Inside a pytest process that depends on test order, so it is tested here, where nothing has measured yet:

  A (CSF_CHASE=0) and B (CSF_CHASE=1): step(600) from tick 0 as one call, then step(200); B measures inside its first call.
  C (CSF_CHASE=1) and D (CSF_CHASE=0), created after B has decided: step(8), step(400) - bench.py's timed engine; C takes B's
  decision over without measuring.

After every call both engines of a pair must hold the same states, destination pointers, navigation states, forces, force parts and
integrator states to the last bit, with no status flag and no dropped near pair.  Prints one JSON object: the checks that failed,
the decision, tick counts, and - not checked - how long the host took to return from B's step(600) and how long the device then
still needed (the queue the measurement began behind).  (The measurement's first side-by-side tick finds its warm-up pair launch
done: the upload of a population of this kind runs it while the host waits anyway - tick.inc: chase_alloc, which orders it behind
every tick queued on the main stream where it does run later.)"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from cyclistsocialforce_amd import engine as csf_engine, parameters  # noqa: E402
from oracle import csf_oracle as orc  # noqa: E402
from test_gpu_chase import crowd  # noqa: E402

CASES = {"twod": (16384, 200.0, 0), "invpend": (16384, 200.0, 0), "planarpoint": (8192, 140.0, 1)}


def make(chase, model, s0, off, dq, rule):
    os.environ["CSF_CHASE"] = str(chase)                  # (read once per engine, in csf_create)
    e = csf_engine.Engine(parameters.default_pod(model, priority_rule=rule), s0.shape[0] + 256)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(s0.shape[0]), off, dq, reset=True)
    return e


def compare(tag, a, b, failed):
    """what tests/test_gpu_chase.py::same compares; the names of what differs are appended to `failed`"""
    sa, pa, za, ta = a.state(with_nav=True)
    sb, pb, zb, tb = b.state(with_nav=True)
    xa, ya, ra = a.integrator_state()
    xb, yb, rb = b.integrator_state()
    checks = {"tick": ta == tb, "state": np.array_equal(sa, sb), "dest_pointer": np.array_equal(pa, pb), "nav_state": np.array_equal(za, zb),
              "forces": np.array_equal(np.c_[a.forces()], np.c_[b.forces()]),
              "force_parts": np.array_equal(np.c_[a.force_parts()], np.c_[b.force_parts()]),
              "integrator_x": np.array_equal(xa, xb), "integrator_psi": np.array_equal(ya, yb), "integrator_zrid": np.array_equal(ra, rb),
              "status_a": bool((a.status() == 0).all()), "status_b": bool((b.status() == 0).all()),
              "near_dropped_a": a.near_dropped() == 0, "near_dropped_b": b.near_dropped() == 0}
    failed.extend(f"{tag}: {k}" for k, ok in checks.items() if not ok)
    if checks["tick"] and not checks["state"]:
        failed.append(f"{tag}: largest state difference {np.abs(sa - sb).max():.3e}")


def main(model):
    n, box, rule = CASES[model]
    s0, off, dq = crowd(n, box, 11, orc.N_STATES[orc.MODEL_IDS[model]])
    failed, out = [], {"model": model, "n": n}

    a = make(0, model, s0, off, dq, rule)
    b = make(1, model, s0, off, dq, rule)
    a.step(600)
    a.sync()                                              # (A's ticks are done before B's measurement starts)
    t0 = time.perf_counter()
    b.step(600)
    t1 = time.perf_counter()
    b.sync()
    t2 = time.perf_counter()
    out["b_step600_host_ms"], out["b_step600_device_after_ms"] = 1e3 * (t1 - t0), 1e3 * (t2 - t1)
    compare("A/B after step(600)", a, b, failed)
    decided, us = b.chase_calibration()
    out["decided"], out["us_per_tick"] = decided, us
    if decided not in (1, -1) or not us[0] > 0 or not us[1] > 0:
        failed.append(f"B did not measure in its step(600): chase_calibration() = {(decided, us)}")
    measured = b.chase_ticks()                            # the side-by-side period of the measurement (+ what followed a decision for it)
    out["b_chase_ticks_600"] = measured
    if not 56 <= measured <= 600:
        failed.append(f"B's step(600) ran {measured} side-by-side ticks: no side-by-side period of 64 ticks was measured")
    if a.chase_ticks() != 0:
        failed.append(f"A (CSF_CHASE=0) ran {a.chase_ticks()} side-by-side ticks")
    a.step(200)
    b.step(200)
    compare("A/B after step(200)", a, b, failed)
    out["b_chase_ticks"] = b.chase_ticks()
    if decided == 1 and b.chase_ticks() < 150:
        failed.append(f"B decided side by side and ran {b.chase_ticks()} side-by-side ticks after 800")
    if decided == -1 and b.chase_ticks() != measured:
        failed.append(f"B decided in turn and ran {b.chase_ticks() - measured} side-by-side ticks after its decision")
    if b.chase_calibration() != (decided, us):
        failed.append(f"B's decision changed: {b.chase_calibration()} after {(decided, us)}")

    c = make(1, model, s0, off, dq, rule)
    d = make(0, model, s0, off, dq, rule)
    for k in (8, 400):
        c.step(k)
        d.step(k)
        compare(f"C/D after step({k})", c, d, failed)
    out["c_calibration"], out["c_chase_ticks"] = c.chase_calibration(), c.chase_ticks()
    if c.chase_calibration() != (decided, [0.0, 0.0]):
        failed.append(f"C did not take B's decision over: {c.chase_calibration()} against {decided}")
    if (c.chase_ticks() >= 350) != (decided == 1) or (decided == -1 and c.chase_ticks() != 0):
        failed.append(f"C ran {c.chase_ticks()} side-by-side ticks of 408 on the decision {decided}")
    for e in (a, b, c, d):
        e.close()
    out["failed"] = failed
    print(json.dumps(out))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "twod")

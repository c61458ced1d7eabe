"""Wrong calls to csf_batch_mid_ticks / csf_batch_launches and the lifetime of a batch with mid-size members, through the raw C
ABI (run as a script in a process of its own by tests/test_gpu_batch_mid.py).  Prints "batch mid abi ok" at the end."""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("CSF_PAIR_VARIANT", None)
from cyclistsocialforce_amd import _ffi, parameters  # noqa: E402
from cyclistsocialforce_amd.engine import Engine  # noqa: E402

E_ARG, E_STATE = -1, -4
L = _ffi.load()


def engine(n, seed=0, model="twod"):
    rng = np.random.default_rng(seed)
    box = max(20.0, 3.0 * np.sqrt(n))
    s0 = np.c_[rng.uniform(0, box, n), rng.uniform(0, box, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 5, n), np.zeros(n)]
    e = Engine(parameters.default_pod(model), n)
    e.add_agents(s0, 5.0)
    dq = np.zeros((n, 2, 3))
    dq[:, 0, :2] = s0[:, :2]
    dq[:, 1, 0], dq[:, 1, 1] = s0[:, 0] + 50 * np.cos(s0[:, 2]), s0[:, 1] + 50 * np.sin(s0[:, 2])
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 2, dq.reshape(-1, 3), reset=True)
    return e


def expect(rc, code, what):
    assert rc == code, f"{what}: {rc} (expected {code})"


n64 = C.c_int64(-7)
a, b, c, lone = engine(40, 1), engine(100, 2), engine(5, 3), engine(64, 4)
expect(L.csf_batch_mid_ticks(None, C.byref(n64)), E_ARG, "mid ticks of NULL")
expect(L.csf_batch_mid_ticks(a._h, None), E_ARG, "mid ticks into NULL")
expect(L.csf_batch_launches(None, C.byref(n64)), E_ARG, "launches of NULL")
expect(L.csf_batch_launches(a._h, None), E_ARG, "launches into NULL")
expect(L.csf_batch_launches(lone._h, C.byref(n64)), E_STATE, "launches of a non-member")
assert n64.value == -7                                  # (a refused call writes nothing)
expect(L.csf_batch_mid_ticks(lone._h, C.byref(n64)), 0, "mid ticks of a non-member")
assert n64.value == 0
Engine.batch_join([a, b, c])
assert a.batch_launches() == 0 and a.batch_mid_ticks() == 0
ta, tb, tc = engine(40, 1), engine(100, 2), engine(5, 3)
Engine.step_batch([a, b, c], 70)
for x, t in ((a, ta), (b, tb), (c, tc)):
    t.step(70)
    assert np.array_equal(x.state(), t.state())
assert a.batch_mid_ticks() == 70 and b.batch_mid_ticks() == 70 and c.batch_mid_ticks() == 0 and c.batch_ticks() == 70
assert a.batch_launches() == b.batch_launches() == c.batch_launches() > 70
lone.step(3)
assert lone.batch_mid_ticks() == 0 and lone.mid_ticks() == 3
b.close()                                               # a destroyed member dissolves the batch
expect(L.csf_batch_launches(a._h, C.byref(n64)), E_STATE, "launches after the batch dissolved")
a.step(5); ta.step(5)
assert np.array_equal(a.state(), ta.state()) and a.batch_mid_ticks() == 70 and a.mid_ticks() == 75
for e in (a, c, lone, ta, tb, tc):
    e.close()

# ---- 50 join / step / leave / destroy rounds with mid-size members: no device memory lost ------------------------------------
try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
free_b, total_b = C.c_size_t(0), C.c_size_t(0)


def free_bytes():
    assert hip.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
    return free_b.value


# (free bytes after round 10 against free bytes after round 50, as tests/batch_abi_child.py does it, and not against the value in
# front of round 1: the runtime's allocator keeps pools that fill during the first rounds - code objects, staging, the streams'
# queues - and are not given back; a leak of a batch's tables or of an engine would show as a loss per round)
seen = []
for r in range(50):
    es = [engine(33 + 11 * ((r + k) % 6), seed=r * 7 + k, model=("twod", "planarpoint")[k % 2]) for k in range(4)] + [engine(3, seed=r)]
    Engine.batch_join(es)
    Engine.step_batch(es, 66)
    outs = [(np.zeros((e.n, e.ns)), None, None, None, None) for e in es]
    Engine.step_batch_into(es, 2, outs)
    if r % 2:
        Engine.batch_leave(es)
    assert all(e.batch_mid_ticks() == 68 for e in es[:4]) and es[4].batch_ticks() == 68
    for e in es:
        e.close()
    if r in (9, 49):
        seen.append(free_bytes())
lost = seen[0] - seen[1]
print("free bytes after round 10 and round 50:", seen, "lost:", lost)
assert lost <= 2 << 20, lost
print("batch mid abi ok")

"""Wrong calls and the lifetime of a batch of engines, through the raw C ABI (run as a script in a process of its own by
tests/test_gpu_batch.py, so that a crash is a failed test and not the end of the test run).  Prints "batch abi ok" at the end."""
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


def engine(n=4, seed=0):
    rng = np.random.default_rng(seed)
    s0 = np.c_[rng.uniform(0, 12, n), rng.uniform(0, 12, n), rng.uniform(-np.pi, np.pi, n), rng.uniform(3, 5, n), np.zeros(n)]
    e = Engine(parameters.default_pod("twod"), n)
    e.add_agents(s0, 5.0)
    dq = np.zeros((n, 2, 3))
    dq[:, 0, :2] = s0[:, :2]
    dq[:, 1, 0], dq[:, 1, 1] = s0[:, 0] + 50 * np.cos(s0[:, 2]), s0[:, 1] + 50 * np.sin(s0[:, 2])
    e.set_dest_queue(np.arange(n), np.arange(n + 1) * 2, dq.reshape(-1, 3), reset=True)
    return e


def arr(engines):
    return (C.c_void_p * len(engines))(*[None if e is None else e._h for e in engines])


def step(engines, k=1, count=None):
    return L.csf_step_batch(arr(engines), len(engines) if count is None else count, k)


def expect(rc, code, what):
    assert rc == code, f"{what}: {rc} (expected {code})"


# ---- wrong calls: refused with the right code and nothing changed --------------------------------------------------------
a, b, c, d = engine(seed=1), engine(seed=2), engine(seed=3), engine(seed=4)
ta, tb, tc = engine(seed=1), engine(seed=2), engine(seed=3)
expect(L.csf_batch_join(None, 2), E_ARG, "join NULL")
expect(L.csf_batch_join(arr([a, b]), 0), E_ARG, "join count 0")
expect(L.csf_batch_join(arr([a, b]), -3), E_ARG, "join count < 0")
expect(L.csf_batch_join(arr([a, None]), 2), E_ARG, "join NULL member")
expect(L.csf_batch_join(arr([a, b, a]), 3), E_ARG, "join duplicate")
expect(step([a, b]), E_STATE, "step before join")
assert a.batch_ticks() == 0 and a.tick == 0 and b.tick == 0
L.csf_comm_init_loopback.argtypes = [C.POINTER(C.c_void_p), C.c_int32]
g1, g2 = engine(seed=5), engine(seed=5)
assert L.csf_comm_init_loopback(arr([g1, g2]), 2) == 0
expect(L.csf_batch_join(arr([c, g1]), 2), E_STATE, "join a loopback member")
Engine.batch_join([a, b, c])
expect(L.csf_batch_join(arr([c, d]), 2), E_STATE, "join an engine already in a batch")
assert d.batch_ticks() == 0
expect(L.csf_comm_init_loopback(arr([c, d]), 2), E_STATE, "loopback of a batch member")
expect(L.csf_step_batch(None, 3, 1), E_ARG, "step NULL")
expect(step([a, b, c], count=0), E_ARG, "step count 0")
expect(step([a, b, c], k=-1), E_ARG, "step n_ticks < 0")
expect(step([a, b, a]), E_ARG, "step duplicate")
expect(step([a, c, b]), E_ARG, "step wrong order")
expect(step([a, b]), E_ARG, "step part of the batch")
expect(step([a, b, c, d]), E_STATE, "step with a non-member")
expect(step([d, a, b]), E_STATE, "step a non-member first")
assert all(e.tick == 0 for e in (a, b, c, d)) and a.batch_ticks() == 0
expect(L.csf_step_batch_get_tick(arr([a, b, c]), 3, 1, None), E_ARG, "get_tick without outputs")
assert L.csf_last_error(a._h)
# after the refusals the batch still steps, bit for bit as the twins
Engine.step_batch([a, b, c], 10)
for t in (ta, tb, tc):
    t.step(10)
for x, t in ((a, ta), (b, tb), (c, tc)):
    assert np.array_equal(x.state(), t.state())
    assert x.batch_ticks() == 10

# ---- a destroyed member: the others go on alone, a batch call fails with CSF_E_STATE -----------------------------------------
b.close()
tb.close()
expect(step([a, c]), E_STATE, "step a dissolved batch")
expect(L.csf_batch_leave(arr([a, c]), 2), E_STATE, "leave a dissolved batch")
a.step(5); c.step(5); ta.step(5); tc.step(5)
for x, t in ((a, ta), (c, tc)):
    assert np.array_equal(x.state(), t.state())
    assert x.batch_ticks() == 10 and x.small_ticks() == 15
Engine.batch_join([c, a])                          # (they may join again)
Engine.step_batch([c, a], 3)
ta.step(3); tc.step(3)
assert np.array_equal(a.state(), ta.state()) and np.array_equal(c.state(), tc.state()) and a.batch_ticks() == 13
Engine.batch_leave([c, a])
expect(step([c, a]), E_STATE, "step after leave")
for e in (a, c, d, ta, tc, g1, g2):
    e.close()

# ---- 100 join / step / leave / destroy rounds: no device memory lost ---------------------------------------------------------
try:
    hip = C.CDLL("libamdhip64.so")
except OSError:
    hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
free_b, total_b = C.c_size_t(0), C.c_size_t(0)


def free_bytes():
    assert hip.hipMemGetInfo(C.byref(free_b), C.byref(total_b)) == 0
    return free_b.value


seen = []
for r in range(100):
    es = [engine(n=1 + (r + k) % 8, seed=r * 7 + k) for k in range(6)]
    Engine.batch_join(es)
    Engine.step_batch(es, 4)
    outs = [(np.zeros((e.n, 5)), None, None, None, None) for e in es]
    Engine.step_batch_into(es, 2, outs)
    if r % 2:
        Engine.batch_leave(es)
    assert all(e.batch_ticks() == 6 for e in es)
    for e in es:
        e.close()
    if r in (9, 99):
        seen.append(free_bytes())
lost = seen[0] - seen[1]
print("free bytes after round 10 and round 100:", seen, "lost:", lost)
assert lost <= 2 << 20, lost
print("batch abi ok")

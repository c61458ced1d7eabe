"""Cases of tests/test_gpu_wg_order.py.  run(name) steps the case's engine under the knobs of the environment and returns what
is compared; `python wg_order_common.py NAME OUT.npz` does so in a process of its own (the reference: CSF_WG_ORDER=0)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def crowd(n, box, seed, ns=5):
    rng = np.random.default_rng(seed)
    s0 = np.zeros((n, ns))
    s0[:, 0] = rng.uniform(0, box, n); s0[:, 1] = rng.uniform(0, box, n)
    s0[:, 2] = rng.uniform(-np.pi, np.pi, n); s0[:, 3] = rng.uniform(3, 6, n)
    d = np.array([50.0, 99.0, 100.0])
    dq = np.zeros((n, 4, 3))
    dq[:, 0, 0] = s0[:, 0]; dq[:, 0, 1] = s0[:, 1]
    dq[:, 1:, 0] = s0[:, 0, None] + d[None, :] * np.cos(s0[:, 2])[:, None]
    dq[:, 1:, 1] = s0[:, 1, None] + d[None, :] * np.sin(s0[:, 2])[:, None]
    return s0, np.arange(n + 1) * 4, dq.reshape(-1, 3)


# name: (n, box, seed, priority rule, pod keywords, environment of the case, stretches of ticks)
CASES = {
    "headline_8192": (8192, 140.0, 21, 0, {}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "0"}, (1, 69, 70)),
    "ragged_8200": (8200, 140.0, 22, 0, {}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "0"}, (1, 20)),
    "p2r_4096": (4096, 100.0, 23, 1, {}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "0"}, (1, 20)),
    "crowd_in_turn": (4096, 45.0, 11, 0, {"hfov": 4.0}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "0"}, (300,)),
    "crowd_side_by_side": (4096, 45.0, 11, 0, {"hfov": 4.0}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "2"}, (300,)),
    "population_changes": (8192, 140.0, 24, 0, {}, {"CSF_WG_ORDER_TICKS": "4", "CSF_CHASE": "0"}, (6, 6, 6, 6)),
    # the shipped defaults on a grid they act on (512 groups x 8 chunks = 4 096 workgroups): no knob of the order is set
    "defaults_16384": (16384, 200.0, 25, 0, {}, {}, (1, 2, 5)),
}


def snapshot(e, out, tag):
    s, ptr, zn, tick = e.state(with_nav=True)
    out[f"{tag}_state"] = s
    out[f"{tag}_ptr"] = ptr
    out[f"{tag}_nav"] = zn
    out[f"{tag}_tick"] = np.array([tick])
    out[f"{tag}_forces"] = np.c_[e.forces()]
    c, name = e.count_pairs(detail=True)
    assert name == "pair_cull_kernel", name
    out[f"{tag}_counters"] = np.array([c[k] for k in ("evaluated", "tested", "full_passes", "partial_passes")], dtype=np.int64)
    out[f"{tag}_near_dropped"] = np.array([e.near_dropped()])
    out[f"{tag}_status"] = np.asarray(e.status())


def run(name, inspect=None, setenv=None):
    """inspect(engine, stretch index): called after every stretch (the in-process side looks at the tables there); setenv: how the
    case's knobs get into the environment (a test passes monkeypatch.setenv, so that nothing outlives it)"""
    setenv = setenv or os.environ.__setitem__
    from cyclistsocialforce_amd import parameters
    from cyclistsocialforce_amd.engine import Engine

    n, box, seed, rule, kw, env, stretches = CASES[name]
    for k, v in env.items():
        setenv(k, v)
    setenv("CSF_PAIR_VARIANT", "0")
    if name != "defaults_16384":
        setenv("CSF_WG_ORDER_MIN", "0")  # (these grids are one round of the device's slots and less: by default they keep index order)
    pod = parameters.default_pod("twod", priority_rule=rule, **kw)      # (the knobs are read in csf_create: the environment is set by now)
    s0, off, dq = crowd(n, box, seed)
    e = Engine(pod, n + 512)
    e.add_agents(s0, 5.0)
    e.set_dest_queue(np.arange(n), off, dq, reset=True)
    out = {}
    rng = np.random.default_rng(seed + 100)
    for k, t in enumerate(stretches):
        if name == "population_changes" and k == 1:      # departures and arrivals between ticks
            e.remove_agents(np.sort(rng.choice(n, 40, replace=False)))
            a0, aoff, adq = crowd(40, box, seed + 1)
            e.add_agents(a0, 5.0)
            e.set_dest_queue(np.arange(n - 40, n), aoff, adq, reset=True)
        if name == "population_changes" and k == 2:      # states pushed from the host
            idx = np.sort(rng.choice(n, 64, replace=False))
            s = e.state()[idx]
            s[:, 0] += 0.25
            e.push_state(idx, s)
        if name == "population_changes" and k == 3:      # departures only: the grid shrinks below a whole last group
            e.remove_agents(np.arange(0, 300, 3))
        e.step(t)
        snapshot(e, out, f"s{k}")
        if inspect is not None:
            inspect(e, k)
    e.close()
    return out


if __name__ == "__main__":
    np.savez(sys.argv[2], **run(sys.argv[1]))

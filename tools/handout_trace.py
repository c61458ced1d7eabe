#!/usr/bin/env python3
"""How long does a workgroup of the pair kernel wait for its last wave?  (measurement aid; reads what tools/block_trace.py run wrote)

    python3 tools/handout_trace.py trace.bin [waves per workgroup = 8]

Per workgroup: tail = exit of its last wave - mean exit of its waves, and the share of its wave-slot time (waves x (last
exit - first entry)) that passes after a wave's own exit, i.e. slots and LDS held for nothing.  Both for all workgroups
and for those of the LAST ROUND: the workgroups still resident when the launch's last workgroup starts - their end is
the drain of the launch.
"""
import sys

import numpy as np


def figures(path, cw=8):
    w = np.fromfile(path, dtype=np.uint64).reshape(-1, 3)
    w = w[: len(w) // cw * cw].reshape(-1, cw, 3)
    w = w[(w[:, :, 1] > 0).all(axis=1)]
    base = int(w[:, :, 0].min())
    t0 = (w[:, :, 0].astype(np.int64) - base) / 100.0           # microseconds (100 MHz)
    t1 = (w[:, :, 1].astype(np.int64) - base) / 100.0
    # a wave's record is written behind the workgroup's last barrier, so its exit is the exit of the slowest sibling: what
    # counts is when it ran out of receivers (bits 36 .. 63 of the third word: the low 28 bits of the clock at that moment)
    wait = (w[:, :, 1].astype(np.int64) - (w[:, :, 2] >> np.uint64(36)).astype(np.int64)) & ((1 << 28) - 1)
    done = t1 - wait / 100.0
    first, last = t0.min(axis=1), done.max(axis=1)
    tail = last - done.mean(axis=1)
    idle = (last[:, None] - done).sum(axis=1)
    slot = cw * (last - first)
    t1 = done
    last_round = last > first.max()
    out = {"workgroups": len(w), "span_us": float(last.max()), "last_start_us": float(first.max()),
           "wave_us_mean": float((t1 - t0).mean()), "wave_us_p95": float(np.percentile(t1 - t0, 95)), "wave_us_max": float((t1 - t0).max())}
    for name, sel in (("all", np.ones(len(w), bool)), ("last_round", last_round)):
        if not sel.any():     # (a build whose kernel does not write the stamp: every wave seems to wait since the clock's last wrap)
            raise SystemExit(f"{path}: no workgroup is resident when the last one starts - was the trace written by a kernel without the stamp?")
        out[name] = {"workgroups": int(sel.sum()), "life_us_mean": float((last - first)[sel].mean()),
                     "tail_us_mean": float(tail[sel].mean()), "tail_us_p50": float(np.median(tail[sel])),
                     "tail_us_p95": float(np.percentile(tail[sel], 95)), "tail_us_max": float(tail[sel].max()),
                     "idle_share": float(idle[sel].sum() / slot[sel].sum())}
    return out


def main():
    f = figures(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 8)
    print(f"workgroups {f['workgroups']}  launch span {f['span_us']:.1f} us  last workgroup starts at {f['last_start_us']:.1f} us  "
          f"wave life mean {f['wave_us_mean']:.2f} p95 {f['wave_us_p95']:.2f} max {f['wave_us_max']:.2f} us")
    for name in ("all", "last_round"):
        g = f[name]
        print(f"{name:10s} workgroups {g['workgroups']:5d}  life mean {g['life_us_mean']:.2f} us  tail (last exit - mean exit) mean "
              f"{g['tail_us_mean']:.2f} p50 {g['tail_us_p50']:.2f} p95 {g['tail_us_p95']:.2f} max {g['tail_us_max']:.2f} us  "
              f"slot time after a wave's exit {100.0 * g['idle_share']:.1f} %")


if __name__ == "__main__":
    main()

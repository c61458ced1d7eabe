#!/usr/bin/env python3
"""Would starting each source chunk's heaviest workgroups first shorten the pair launch?  (measurement aid; reads what
tools/block_trace.py run wrote)

    python3 tools/wg_order_estimate.py T.bin T2.bin T16.bin [--groups 512] [--waves 8] [--chunks 8] [--turnover 1.4]

T.bin, T2.bin and T16.bin are the traces of the pair launch at ticks t, t + 2 and t + 16 of one population (the engine
writes the trace of its LAST launch: block_trace.py run with TICKS = t, t + 2, t + 16 - the states are bit-reproducible,
so the three processes trace three launches of the same run).  The launch is `chunks` x `groups` workgroups, dispatched
chunk by chunk, `groups` receiver groups in index order inside a chunk.  Reported:

  (a) the spread of workgroup life (first entry of a wave to last exit) inside each chunk;
  (b) how well one launch's lives predict a later launch's: correlation across the lag of 2 and of 16 ticks, over all
      workgroups and inside the chunks (chunk mean removed: only the order INSIDE a chunk is free), and with the count proxy
      28 x tests + 58 x evaluations per workgroup: --costs T.npy T2.npy T16.npy, the cost tables the three launches left in
      Dev::wg_cost (COSTS=T.npy tools/block_trace.py run saves the last launch's, read through csf_wg_order_tables).  The study in
      profiles/wg_order_estimate.txt predates that table: its measurement build stored tests | evaluations << 32 of every wave in
      words 3 W .. 4 W - 1 behind the W wave records, which the committed kernel does not write - that reader is kept for those traces;
  (c) the launch span when the recorded lives are replayed on 256 x 4 slots - every workgroup, in dispatch order, takes the
      slot that frees first, `turnover` us after its predecessor left - in index order and heaviest first inside each chunk,
      the order taken from the EARLIER launch (what the device could know), from the proxy of the earlier launch, and from
      the launch's own lives (the bound no predictor passes).

The replay keeps a workgroup's life whatever its neighbours are: on the device the workgroups of a CU share its issue
slots, so a life recorded beside light neighbours would be longer beside heavy ones.  The replay of the index order is
printed beside the measured span to show how far that matters.
"""
import argparse
import heapq

import numpy as np

SLOTS = 256 * 4


def load(path, groups, cw, chunks=0):
    raw = np.fromfile(path, dtype=np.uint64)
    w = raw[: len(raw) // 3 * 3].reshape(-1, 3)
    if chunks == 0:     # the wave records lead the file: entry <= exit, all within 10 ms (the counts behind them are no such pairs)
        lo = w[0, 0] - min(w[0, 0], np.uint64(1000000))
        ok = (w[:, 0] >= lo) & (w[:, 1] >= w[:, 0]) & (w[:, 1] - lo < np.uint64(2000000))
        nrec = len(ok) if ok.all() else int(np.argmin(ok))
        chunks = nrec // (cw * groups)
        if chunks == 0 or nrec != chunks * cw * groups:
            raise SystemExit(f"{path}: {nrec} wave records are no whole chunks of {groups} workgroups x {cw} waves (give --chunks)")
    nwg = chunks * groups
    r = w[: nwg * cw].reshape(nwg, cw, 3)
    if not (r[:, :, 1] > 0).all():
        raise SystemExit(f"{path}: not {chunks} x {groups} workgroups of {cw} waves")
    base = int(r[:, :, 0].min())
    first = (r[:, :, 0].astype(np.int64).min(axis=1) - base) / 100.0          # microseconds (100 MHz)
    last = (r[:, :, 1].astype(np.int64).max(axis=1) - base) / 100.0
    hw = r[:, 0, 2]
    hwid = hw & np.uint64(0xFFFFFFFF)
    xcc = (hw >> np.uint64(32)) & np.uint64(0xF)
    cu = (((xcc * np.uint64(8) + ((hwid >> np.uint64(13)) & np.uint64(7))) * np.uint64(2) + ((hwid >> np.uint64(12)) & np.uint64(1)))
          * np.uint64(16) + ((hwid >> np.uint64(8)) & np.uint64(0xF))).astype(np.int64)
    cost = None
    nw = nwg * cw
    if len(raw) >= 4 * nw and raw[3 * nw: 4 * nw].any():     # measurement build: tests | evaluations << 32 of every wave
        c = raw[3 * nw: 4 * nw].reshape(nwg, cw)
        cost = (28.0 * (c & np.uint64(0xFFFFFFFF)).astype(np.float64) + 58.0 * (c >> np.uint64(32)).astype(np.float64)).sum(axis=1)
    return {"first": first, "last": last, "life": last - first, "cu": cu, "cost": cost, "chunks": chunks, "groups": groups,
            "span": float(last.max())}


def ranks(v):
    r = np.empty(len(v))
    r[np.argsort(v, kind="stable")] = np.arange(len(v))
    return r


def corr(a, b):
    return float(np.corrcoef(a, b)[0, 1]) if a.std() > 0 and b.std() > 0 else float("nan")


def within(v, chunks, groups):
    m = v.reshape(chunks, groups)
    return (m - m.mean(axis=1, keepdims=True)).ravel()


def heaviest_first(key, chunks, groups):
    """per chunk: the groups by falling key, equal keys in index order (the ranking of the kernel-side proposal)"""
    k = key.reshape(chunks, groups)
    return np.stack([np.argsort(-k[c], kind="stable") for c in range(chunks)])


def replay(life, order, turnover):
    """list scheduling: workgroups in dispatch order (chunk-major, `order` inside a chunk), each on the slot that frees first"""
    chunks, groups = order.shape
    free = [0.0] * SLOTS
    heapq.heapify(free)
    lf = life.reshape(chunks, groups)
    last_start = 0.0
    n = 0
    for c in range(chunks):
        for g in order[c]:
            t = heapq.heappop(free)
            start = t + turnover if n >= SLOTS else t
            last_start = max(last_start, start)
            heapq.heappush(free, start + lf[c, g])
            n += 1
    ends = np.array(free)
    span = float(ends.max())
    return span, float(np.mean(span - ends)), last_start


def measured_idle(tr):
    """launch end - last exit on a CU, mean over the CUs (which of a CU's four slots a workgroup held is not recorded)"""
    last = np.zeros(int(tr["cu"].max()) + 1)
    np.maximum.at(last, tr["cu"], tr["last"])
    last = last[last > 0]
    return float(np.mean(tr["span"] - last))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("traces", nargs=3, help="traces of ticks t, t + 2, t + 16")
    ap.add_argument("--groups", type=int, default=512)
    ap.add_argument("--waves", type=int, default=8)
    ap.add_argument("--chunks", type=int, default=0, help="source chunks of the launch (default: read off the trace)")
    ap.add_argument("--costs", nargs=3, default=None, help="cost tables [chunks, groups] of the three launches (.npy)")
    ap.add_argument("--turnover", type=float, default=1.4, help="us between a workgroup's exit and its successor's entry on a slot")
    a = ap.parse_args()
    t0, t2, t16 = (load(p, a.groups, a.waves, a.chunks) for p in a.traces)
    chunks, groups = t0["chunks"], t0["groups"]
    if a.costs:
        for tr, path in zip((t0, t2, t16), a.costs):
            tr["cost"] = np.load(path).astype(np.float64).reshape(chunks * groups)
    ident = np.tile(np.arange(groups), (chunks, 1))

    print(f"launch: {chunks} chunks x {groups} workgroups of {a.waves} waves; replay on {SLOTS} slots, turnover {a.turnover} us")
    print("\n(a) workgroup life inside each chunk, us")
    print("launch  chunk   mean    std     p5    p50    p95    max   first_entry  last_exit")
    for name, tr in (("t", t0), ("t+2", t2), ("t+16", t16)):
        lf = tr["life"].reshape(chunks, groups)
        for c in range(chunks):
            v = lf[c]
            print(f"{name:6s}  {c:5d}  {v.mean():5.2f}  {v.std():5.2f}  {np.percentile(v, 5):5.2f}  {np.median(v):5.2f}  "
                  f"{np.percentile(v, 95):5.2f}  {v.max():5.2f}   {tr['first'].reshape(chunks, groups)[c].min():8.1f}   "
                  f"{tr['last'].reshape(chunks, groups)[c].max():8.1f}")
        w = within(tr["life"], chunks, groups)
        print(f"{name:6s}  all    mean {tr['life'].mean():.2f}  std {tr['life'].std():.2f}  std inside the chunks {w.std():.2f}  "
              f"measured span {tr['span']:.1f}  last start {tr['first'].max():.1f}  mean idle per CU at the end {measured_idle(tr):.1f}")

    print("\n(b) one workgroup's life across the lag (Pearson / Spearman), all workgroups and inside the chunks (chunk mean removed)")
    for name, later in (("t -> t+2", t2), ("t -> t+16", t16)):
        x, y = t0["life"], later["life"]
        xw, yw = within(x, chunks, groups), within(y, chunks, groups)
        print(f"{name:10s}  all {corr(x, y):.3f} / {corr(ranks(x), ranks(y)):.3f}   inside chunks {corr(xw, yw):.3f} / {corr(ranks(xw), ranks(yw)):.3f}")
    if t0["cost"] is not None:
        print("    life against the count proxy 28 x tests + 58 x evaluations per workgroup")
        for name, src, dst in (("same launch t", t0, t0), ("same launch t+2", t2, t2), ("proxy t -> life t+2", t0, t2), ("proxy t -> life t+16", t0, t16)):
            if src["cost"] is None:
                continue
            x, y = src["cost"], dst["life"]
            xw, yw = within(x, chunks, groups), within(y, chunks, groups)
            print(f"{name:22s}  all {corr(x, y):.3f} / {corr(ranks(x), ranks(y)):.3f}   inside chunks {corr(xw, yw):.3f} / {corr(ranks(xw), ranks(yw)):.3f}")
        for name, later in (("proxy t -> proxy t+2", t2), ("proxy t -> proxy t+16", t16)):
            if later["cost"] is not None:
                xw, yw = within(t0["cost"], chunks, groups), within(later["cost"], chunks, groups)
                print(f"{name:22s}  inside chunks {corr(xw, yw):.3f} / {corr(ranks(xw), ranks(yw)):.3f}")
    else:
        print("    (no count proxy: give --costs)")

    print("\n(c) replay of the recorded lives: span, mean idle per slot at the end, start of the last workgroup (us); gain = index - order")
    for name, tr in (("t+2", t2), ("t+16", t16)):
        s_idx, i_idx, l_idx = replay(tr["life"], ident, a.turnover)
        print(f"launch {name}: measured span {tr['span']:.1f}")
        print(f"  index order                         span {s_idx:6.1f}  idle {i_idx:4.1f}  last start {l_idx:5.1f}")
        cands = [("heaviest first, lives of launch t  ", t0["life"])]
        if t0["cost"] is not None:
            cands.append(("heaviest first, proxy of launch t  ", t0["cost"]))
        if tr["cost"] is not None:
            cands.append(("heaviest first, own proxy (bound)  ", tr["cost"]))
        cands.append(("heaviest first, own lives (bound)  ", tr["life"]))
        cands.append(("lightest first, own lives (worst)  ", -tr["life"]))
        for label, key in cands:
            s, i, l = replay(tr["life"], heaviest_first(key, chunks, groups), a.turnover)
            print(f"  {label} span {s:6.1f}  idle {i:4.1f}  last start {l:5.1f}  gain {s_idx - s:+5.2f}")
        rng = np.random.default_rng(1)
        sp = [replay(tr["life"], np.stack([rng.permutation(groups) for _ in range(chunks)]), a.turnover)[0] for _ in range(8)]
        print(f"  random order inside the chunks (8)  span {np.mean(sp):6.1f}  (min {min(sp):.1f} max {max(sp):.1f}): what the order is worth by chance")
    print("\nturnover sensitivity of the predicted gain (order from the lives of launch t, replayed on launch t+2)")
    for tv in (0.0, 0.7, 1.4, 2.1):
        s_idx = replay(t2["life"], ident, tv)[0]
        s = replay(t2["life"], heaviest_first(t0["life"], chunks, groups), tv)[0]
        print(f"  turnover {tv:3.1f} us: index {s_idx:6.1f}  heaviest first {s:6.1f}  gain {s_idx - s:+5.2f}")


if __name__ == "__main__":
    main()

"""tools/wg_order_estimate.py on synthetic traces (no GPU): the trace reader, the order and the replay do what the study
in profiles/wg_order_estimate.txt relies on."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("wg_order_estimate", os.path.join(ROOT, "tools", "wg_order_estimate.py"))
woe = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(woe)


def _trace(path, first, life, cw, counts=None, slack=64):
    """the file block_trace.py leaves: 3 words per wave (entry, exit, hw id), zeros behind - and, as a measurement build writes
    them, one word of counts per wave behind the records"""
    nwg = len(first)
    rec = np.zeros((nwg, cw, 3), np.uint64)
    rec[:, :, 0] = (5_000_000 + np.round(first * 100)).astype(np.uint64)[:, None]
    rec[:, :, 1] = (5_000_000 + np.round((first + life) * 100)).astype(np.uint64)[:, None]
    rec[:, :, 2] = ((np.arange(nwg) % 16) << 8).astype(np.uint64)[:, None]
    words = [rec.ravel()]
    if counts is not None:
        tests, evals = counts
        words.append(np.repeat(tests.astype(np.uint64) | (evals.astype(np.uint64) << np.uint64(32)), cw))
    words.append(np.zeros(slack, np.uint64))
    np.concatenate(words).tofile(path)


def test_heaviest_first_is_a_stable_permutation():
    rng = np.random.default_rng(0)
    for key in (rng.uniform(0, 30, 3 * 37), np.full(3 * 37, 7.0), np.zeros(3 * 37), rng.integers(0, 3, 3 * 37).astype(float)):
        order = woe.heaviest_first(key, 3, 37)
        assert order.shape == (3, 37)
        k = key.reshape(3, 37)
        for c in range(3):
            assert np.array_equal(np.sort(order[c]), np.arange(37))
            along = k[c][order[c]]
            assert (np.diff(along) <= 0).all()
            same = np.diff(along) == 0
            assert (np.diff(order[c])[same] > 0).all()          # equal keys keep index order


def test_replay_is_list_scheduling():
    # fewer workgroups than slots: everything starts at 0, the span is the longest life, no turnover is paid
    life = np.arange(1.0, 1.0 + 2 * 8)
    ident = np.tile(np.arange(8), (2, 1))
    span, idle, last_start = woe.replay(life, ident, 1.4)
    assert span == 16.0 and last_start == 0.0
    assert np.isclose(idle, (woe.SLOTS * 16.0 - life.sum()) / woe.SLOTS)
    # two rounds of equal lives on every slot: the second round pays the turnover once
    life = np.full(2 * woe.SLOTS, 10.0)
    span, idle, last_start = woe.replay(life, np.tile(np.arange(woe.SLOTS), (2, 1)), 1.5)
    assert np.isclose(span, 21.5) and np.isclose(idle, 0.0) and np.isclose(last_start, 11.5)
    # the order matters and heaviest first is the better one: one long workgroup among short ones, in the last chunk
    life = np.full(2 * woe.SLOTS, 10.0)
    life[-1] = 30.0
    ident = np.tile(np.arange(woe.SLOTS), (2, 1))
    s_idx = woe.replay(life, ident, 0.0)[0]
    s_hf = woe.replay(life, woe.heaviest_first(life, 2, woe.SLOTS), 0.0)[0]
    assert np.isclose(s_idx, 40.0) and np.isclose(s_hf, 40.0)        # (every slot frees at 10: the long one starts then either way)
    life[woe.SLOTS:] = np.linspace(5.0, 15.0, woe.SLOTS)              # ... with slots that free one after another the order decides
    life[:woe.SLOTS] = np.linspace(5.0, 15.0, woe.SLOTS)
    s_idx = woe.replay(life, ident, 0.0)[0]
    s_hf = woe.replay(life, woe.heaviest_first(life, 2, woe.SLOTS), 0.0)[0]
    assert s_hf < s_idx


def test_load_reads_records_and_counts(tmp_path):
    rng = np.random.default_rng(1)
    chunks, groups, cw = 3, 20, 8
    first = np.sort(rng.uniform(0, 50, chunks * groups))
    life = rng.uniform(10, 30, chunks * groups)
    tests = rng.integers(1000, 50000, chunks * groups)
    evals = rng.integers(100, 9000, chunks * groups)
    p = str(tmp_path / "with_counts.bin")
    _trace(p, first, life, cw, (tests, evals))
    for ch in (0, chunks):          # read off the trace, and given
        tr = woe.load(p, groups, cw, ch)
        assert tr["chunks"] == chunks
        assert np.allclose(tr["life"], life, atol=0.011) and np.allclose(tr["first"], first - first.min(), atol=0.011)
        assert np.allclose(tr["cost"], cw * (28.0 * tests + 58.0 * evals))
    p = str(tmp_path / "plain.bin")
    _trace(p, first, life, cw)
    tr = woe.load(p, groups, cw)
    assert tr["cost"] is None and tr["chunks"] == chunks and np.isclose(tr["span"], (first - first.min() + life).max(), atol=0.011)


def test_report_runs(tmp_path, capsys, monkeypatch):
    rng = np.random.default_rng(2)
    chunks, groups, cw = 2, 16, 4
    base = rng.uniform(15, 25, chunks * groups)
    paths = []
    for i in range(3):
        life = base + rng.normal(0, 0.5, chunks * groups)
        p = str(tmp_path / f"t{i}.bin")
        _trace(p, np.repeat(np.arange(chunks) * 10.0, groups), life, cw)
        np.save(str(tmp_path / f"c{i}.npy"), (life * 1000).astype(np.uint32).reshape(chunks, groups))
        paths.append(p)
    costs = [str(tmp_path / f"c{i}.npy") for i in range(3)]
    monkeypatch.setattr("sys.argv", ["wg_order_estimate.py", *paths, "--groups", str(groups), "--waves", str(cw), "--costs", *costs])
    woe.main()
    out = capsys.readouterr().out
    assert "(a) workgroup life" in out and "(b) one workgroup's life" in out and "(c) replay" in out
    assert "heaviest first, proxy of launch t" in out

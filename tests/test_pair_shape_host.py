"""Which kernel a pair launch takes (csrc/csf_pair.hip: pair_shape), on the host: csf_pair_shape_of answers with the very function
every launch, the order tables, the gate of the side-by-side tick and the candidate lists ask.  No device is needed.

tests/golden/pair_shape_table.npz holds what the if-chains that pair_shape replaced chose, for the whole lattice of the words they
read: priority to the right x 1 / 3 / 300 parameter sets x (has_bike, model_mask) x Bicycle / TwoD x classify x recs_valid x
pair_variant 0 / 1 / 2 x recv_binned x rpb 16 / 32 x wide x reach x order tables given x the segmented one-grid launch - 27 648 rows,
69 distinct answers.  How it was made: the launch functions of the commit before pair_shape (launch_pair, launch_cull,
launch_cull_dyn, launch_pair_segments, pair_order_groups, pair_kernel_name) were compiled unmodified as host code, over function
templates with the kernels' parameter lists that record their own template arguments and a launch macro that records grid and
block; the program ran over the lattice with 1, 16, 17 and 4 097 receivers and 3 source chunks (5 for the segmented grid), and
the rows of the two retired shapes (static hand-out, 8 receivers per workgroup) were dropped.  `ids` has one axis per word, in the
order of meta["axes"]; shapes[id] is meta["fields"]: the kernel family, its template arguments (0 where the family has none),
receivers and threads per workgroup, the name pair_kernel_name gave (the launched kernel's for the segmented grid) and the
receivers per group of pair_order_groups (0: no tables for this launch)."""
import ctypes as C
import itertools
import json
import os

import numpy as np
import pytest

from cyclistsocialforce_amd import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = np.load(os.path.join(HERE, "golden", "pair_shape_table.npz"))
META = json.loads(str(TABLE["meta"]))
AXES = META["axes"]
NLOC = (1, 16, 17, 4097)
CULL = (4, 5)


def words_of(index, nloc):
    v = {}
    for (name, values), i in zip(AXES, index):
        if "," in name:
            v.update(zip(name.split(","), values[i]))
        else:
            v[name] = values[i]
    v["nloc"] = nloc
    w = (C.c_int32 * _ffi.PAIR_SHAPE_IN)()
    for k, name in enumerate(_ffi.PAIR_SHAPE_INPUTS):
        w[k] = v[name]
    return w


def test_table_covers_the_lattice():
    assert TABLE["ids"].shape == tuple(len(values) for _, values in AXES) and TABLE["ids"].size == 27648
    assert TABLE["ids"].max() == len(TABLE["shapes"]) - 1 == 68
    assert TABLE["shapes"].shape[1] == len(META["fields"])
    families = set(int(f) for f in TABLE["shapes"][:, 0])
    assert families == {0, 1, 2, 3, 4, 5}


# one case per priority rule and launch entry: 6 912 rows each
@pytest.mark.parametrize("segments", [0, 1])
@pytest.mark.parametrize("p2r", [0, 1])
def test_every_row_takes_the_recorded_shape(p2r, segments):
    lib = _ffi.load()
    assert hasattr(lib, "csf_pair_shape_of")
    ids = TABLE["ids"]
    rows = 0
    for index in itertools.product(*(range(n) for n in ids.shape)):
        if index[0] != p2r or index[-1] != segments:
            continue
        rows += 1
        want = dict(zip(META["fields"], (int(x) for x in TABLE["shapes"][ids[index]])))
        for nloc in NLOC:
            got = _ffi.pair_shape_of(lib, words_of(index, nloc))
            where = (index, nloc, got, want)
            assert got["family"] == want["family"] and got["name"] == META["names"][want["name"]], where
            assert got["order_groups"] == (-(-nloc // want["order_unit"]) if want["order_unit"] else 0), where
            if want["family"] == 0:          # nothing is launched
                continue
            for f in ("field", "rw", "p2r", "per_group", "threads"):
                assert got[f] == want[f], (f,) + where
            if want["family"] in CULL:
                for f in ("classify", "binr", "ord", "reach", "rpb", "cw"):
                    assert got[f] == want[f], (f,) + where
                assert got["tile"] == 256 * want["cw"] and got["threads"] == 64 * want["cw"] and got["per_group"] == want["rpb"], where
            assert got["grid_x"] == -(-nloc // got["per_group"]), where
    assert rows == 6912


def test_only_the_instances_that_exist():
    """(receivers, reach test, waves) of every cull-family answer is one of the rows launch_cull lists"""
    s = TABLE["shapes"]
    f = META["fields"].index
    cull = s[np.isin(s[:, f("family")], CULL)]
    seen = set((int(r[f("classify")]), int(r[f("rpb")]), int(r[f("reach")]), int(r[f("cw")])) for r in cull)
    assert seen == {(1, 16, 1, 8), (1, 32, 1, 8), (1, 16, 1, 4), (1, 32, 1, 4), (1, 32, 0, 8), (1, 16, 0, 4), (1, 32, 0, 4), (0, 16, 0, 4), (0, 32, 0, 4)}
    seg = s[s[:, f("family")] == 5]
    assert set((int(r[f("rpb")]), int(r[f("reach")]), int(r[f("cw")])) for r in seg) == {(16, 1, 8), (32, 1, 8)}


def test_other_values_of_rpb_mean_16():
    lib = _ffi.load()
    index = [0] * len(AXES)
    index[[n for n, _ in AXES].index("model")] = 1
    for rpb, want in ((0, 16), (8, 16), (16, 16), (24, 16), (32, 32), (64, 16)):
        w = words_of(index, 100)
        w[_ffi.PAIR_SHAPE_INPUTS.index("rpb")] = rpb
        got = _ffi.pair_shape_of(lib, w)
        assert got["family"] == 4 and got["rpb"] == got["per_group"] == want, (rpb, got)


def test_bad_arguments():
    lib = _ffi.load()
    w = (C.c_int32 * _ffi.PAIR_SHAPE_IN)()
    o = (C.c_int32 * _ffi.PAIR_SHAPE_OUT)()
    assert lib.csf_pair_shape_of(None, o, None) == -1 and lib.csf_pair_shape_of(w, None, None) == -1
    assert lib.csf_pair_shape_of(w, o, None) == _ffi.PAIR_SHAPE_OUT

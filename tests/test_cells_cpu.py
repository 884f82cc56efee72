"""The restatement of br_cells and of br_dedup's "cell_source" (tests/cells_cases.py) pinned by hand, and the conditions that
tests/test_gpu_cells.py relies on for its inputs.  No GPU."""
import functools

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests import cells_cases as cc
from tests import dedup_cases as dc


def _rec(name, aux=b""):
    return bamio.bam_record(name, 0, 10, dc.cig("30M"), 30, flag=0, aux=aux)


def test_one_cell_by_hand():
    es, slots = [(0, 3, (0,)), (1, 2, (0, 1))], [0, 1]   # {A}: 3, {A, B}: 2
    assert cc.unique_cell(es, slots) == [3.0, 0.0]
    model = {"cells": [b"AC"], "name_cell": None, "entries": [es], "slots": [slots]}
    u = cc.matrix_of(model, "unique")
    assert list(u["feature"]) == [0] and list(u["value"]) == [3.0] and list(u["off"]) == [0, 1]   # the slot that ends at 0 is gone
    assert (int(u["names"][0]), int(u["unique"][0]), int(u["multi"][0]), int(u["features"][0])) == (5, 3, 2, 1)
    f = cc.matrix_of(model, "uniform")
    assert list(f["value"]) == [4.0, 1.0] and list(f["iterations"]) == [1]
    theta, it = cc.em_cell(es, slots, 1, 0.0)
    assert theta == [4.0, 1.0] and it == 1
    theta, it = cc.em_cell(es, slots, 2, 0.0)
    assert theta == [4.0 * (0.75 + 0.4), 0.4] and it == 2
    theta, it = cc.em_cell(es, slots, 10000, 1e-2)
    assert it < 10000 and abs(theta[0] - 5) < 0.05 and theta[1] < 0.05 and abs(sum(theta) - 5) < 1e-9
    theta, it = cc.em_cell(es, slots, 7, 0.0)   # tolerance 0 never stops early
    assert it == 7


def test_em_edges():
    # an entry whose features all sit at 0: q = 0, not a division by zero
    theta, it = cc.em_cell([(0, 2, (3,))], [3], 3, 0.0)
    assert theta == [2.0] and it == 3
    # a class of two transcripts of one feature is an entry of one feature
    model = cc.model_of([b"AA", b"AA"], np.array([0, 1], np.uint32), [(4, 5), (4,)], cc.TX_FEATURE)
    assert model["entries"] == [[(0, 1, (2,)), (1, 1, (2,))]] and model["slots"] == [[2]]
    assert list(cc.matrix_of(model, "unique")["value"]) == [2.0]


def test_barcode_parsing():
    for name, want in ((b"r_ACGT_TTT", (b"ACGT", "")), (b"r_ACGT", (None, "none")), (b"plain", (None, "none")), (b"a_b_ACGT_TTT", (b"ACGT", "")),
                       (b"r__TTT", (None, "none")), (b"r_" + b"A" * 32 + b"_T", (b"A" * 32, "")), (b"r_" + b"A" * 33 + b"_T", (None, "too_long")),
                       (b"_AC_", (b"AC", "")), (b"__", (None, "none"))):
        assert cc.barcode_of_record(_rec(name)) == want, name
    assert cc.barcode_of_record(_rec(b"r:AC:T"), sep=b":") == (b"AC", "")
    for aux, want in ((b"CBZ" + b"ACGT\0", (b"ACGT", "")), (b"NHC\x01CBZ" + b"AC\0", (b"AC", "")), (b"CBA" + b"x" + b"CBZAC\0", (b"AC", "")),
                      (b"CBZ\0", (None, "none")), (b"NHC\x01", (None, "none")), (b"XSi\x01\x02", (None, "bad_aux")), (b"CBZAC", (None, "bad_aux")),
                      (b"CBZ" + b"A" * 33 + b"\0", (None, "too_long")), (b"CBZAC\0XSi\x01", (b"AC", ""))):
        assert cc.barcode_of_record(_rec(b"r_TT_GG", aux), "tag") == want, aux
    assert cc.barcode_of_record(_rec(b"r", b"XYZ" + b"AC\0"), "tag", tag=b"XY") == (b"AC", "")
    groups = [[_rec(b"a_AC_T")], [], [_rec(b"b_" + b"C" * 33 + b"_T")], [_rec(b"c")]]
    bcs, cnt = cc.barcodes_of(groups)
    assert bcs == [b"AC", None, None, None] and cnt == {"no_barcode": 2, "too_long": 1, "bad_aux": 0}


def test_cells_are_numbered_by_length_then_bytes():
    model = cc.model_of([b"TT", b"A", b"AAA", b"AC", None, b"G", b"TT"], np.array([0, 0, 1, 0, 0, cc.NONE, 1], np.uint32), [(0,), (0, 2)], cc.TX_FEATURE)
    assert model["cells"] == [b"A", b"AC", b"TT", b"AAA"]
    assert list(model["name_cell"]) == [2, 0, 3, 1, cc.NONE, cc.NONE, 2]
    assert model["entries"][2] == [(0, 1, (0,)), (1, 1, (0, 1))]


def test_per_cell_groups_are_the_molecules_of_signature_and_barcode():
    run = cc.dedup_run()
    groups = dc.records_of(run)
    umis, _ = dc.umis_of(groups)
    bcs, _ = cc.barcodes_of(groups)
    for method in ("directional", "unique"):
        rep, gf = cc.per_cell_molecules(method, groups, umis, bcs)
        plain = dc.molecules_of(method, dc.signatures_of(groups), umis)
        assert not np.array_equal(rep, plain)   # the barcode decides something
        # the hand-made head of the run
        assert list(gf[:10]) == [0, 1, 0, 0, 1, 1, 1, 7, 7, 7]
        want = [0, 1, 0, 0, 4, 4, 4, 7, 7, 7] if method == "directional" else [0, 1, 0, 3, 4, 4, 4, 7, 7, 7]
        if method == "directional":
            want[1] = 4   # GGGGTTTT: ACGTAA x 3 takes ACGTAC x 1
        assert list(rep[:10]) == want, method
        # by definition: umi_tools' method inside every (signature, barcode) group on its own
        sigs = dc.signatures_of(groups)
        for key in set((s, b or b"") for s, b in zip(sigs, bcs) if s is not None):
            mine = [i for i in range(len(run)) if sigs[i] == key[0] and (bcs[i] or b"") == key[1]]
            alone = dc.molecules_of(method, [sigs[i] for i in mine], [umis[i] for i in mine])
            assert [mine[r] for r in alone] == [int(rep[i]) for i in mine]


@functools.lru_cache(maxsize=None)
def _model(kind):
    run = {"standard": cc.standard_run, "stopping": cc.stopping_run}[kind]()
    groups = dc.records_of(run)
    bcs, cnt = cc.barcodes_of(groups)
    name_cls, classes = cc.classes_of(groups)
    return run, bcs, cnt, cc.model_of(bcs, name_cls, classes, cc.TX_FEATURE)


def test_the_standard_input_reaches_every_route():
    run, bcs, cnt, model = _model("standard")
    assert 64 < len(model["cells"]) <= 80
    shape = [(len(s), sum(len(fs) for _, _, fs in es), len(es)) for es, s in zip(model["entries"], model["slots"])]   # slots, pairs, entries
    assert sum(1 for s in shape if s[2] == 1) >= 30
    assert any(s[0] == 64 and s[1] == 64 for s in shape) and any(s[0] == 65 for s in shape)
    assert any(s[0] <= 64 and s[1] == 65 for s in shape)
    assert any(max(sum(1 for _, _, fs in es if f in fs) for f in sl) > 64 for es, sl in zip(model["entries"], model["slots"]))
    assert any(max(len(fs) for _, _, fs in es) > 64 for es in model["entries"])
    # at "lds_bytes" cc.LDS_LOW a cell stays in LDS and another goes to HBM: 8 (2 slots + entries) + 64
    big = [8 * (2 * s[0] + s[2]) + 64 for s in shape if s[0] > 64 or s[1] > 64]
    assert any(x <= cc.LDS_LOW for x in big) and any(x > cc.LDS_LOW for x in big) and all(x <= 65536 for x in big)
    assert cnt == {"no_barcode": 5, "too_long": 1, "bad_aux": 0}
    assert any(b is not None and len(b) == 32 for b in model["cells"])
    assert sum(1 for nm in run if not nm["rows"]) == 1
    groups_t = dc.records_of(cc.tagged(run))
    bt, ct = cc.barcodes_of(groups_t, "tag")
    assert ct["bad_aux"] == 1 and ct["too_long"] == 1 and sum(a != b for a, b in zip(bcs, bt)) == 1
    # every value of every mode is an exact integer sum in "unique", and multi-feature entries exist
    u = cc.matrix_of(model, "unique")
    assert u["multi"].sum() > 0 and np.array_equal(u["value"], np.round(u["value"])) and (u["features"] < [len(s) for s in model["slots"]]).any()


@pytest.mark.parametrize("mode,iters", [("uniform", 1), ("em", 40)])
def test_the_spread_of_the_standard_input(mode, iters):
    _, _, _, model = _model("standard")
    ref, s = cc.spread_of(model, mode, iters)
    print("%s: spread s over three summation orders after %d iterations = %.3e" % (mode, iters, s))
    assert 0 < s < 1e-9
    assert list(ref["iterations"]) == [iters] * len(model["cells"])


def test_the_stopping_input_stops_at_the_same_iteration_in_every_order():
    _, _, _, model = _model("stopping")
    runs = [cc.matrix_of(model, "em", order=o) for o in ("forward", "reversed", 12345)]
    for other in runs[1:]:
        assert np.array_equal(other["iterations"], runs[0]["iterations"])
    its = runs[0]["iterations"]
    assert len(set(its.tolist())) >= 5 and its.max() < 10000 and its.min() >= 2
    # rounding does not decide any of them: rel of the stopping iteration and of the one before lie 1e-9 clear of the tolerance
    for es, slots, n in zip(model["entries"], model["slots"], its):
        for k, stops in ((int(n) - 1, False), (int(n), True)):
            a, _ = cc.em_cell(es, slots, k - 1, 0.0)
            b, _ = cc.em_cell(es, slots, k, 0.0)
            rel = max(abs(y - x) / y for x, y in zip(a, b) if y > 1e-8)
            assert (rel < 1e-2 - 1e-9) if stops else (rel > 1e-2 + 1e-9)


def test_the_wrapper_is_there():
    for name in ("add_host", "add_device", "add_last", "barcodes", "finish", "cell_barcodes", "name_cells", "matrix", "cell_stats", "stats"):
        assert hasattr(lib.Cells, name), name
    assert lib.Cells.MODES == cc.MODES and lib.Cells.SOURCES == cc.SOURCES and lib.Dedup.CELL_SOURCES == {"none": 0, "name": 1, "tag": 2}
    assert len(lib.Cells.STATS) == 16

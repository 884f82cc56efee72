"""--cells on the GPU: br_cells' barcodes, cells, sparse structure, values and per-cell numbers, and br_dedup's per-cell position
groups, against the tests' restatement of the definitions (tests/cells_cases.py; tests/test_cells_cpu.py pins it on the CPU and checks
the inputs used here).  Integers and structure bit for bit through every way in; the float values by the rule of
tests/test_gpu_quant.py::_assert_em_to, with the restatement's own spread over three summation orders as the yardstick."""
import functools
import os
import re

import numpy as np
import pytest

from bramble_amd import lib
from tests import cells_cases as cc
from tests import dedup_cases as dc

pytestmark = pytest.mark.gpu

INVALID = -1
HOWS = ("host", "host3", "dev1", "dev3")
EM_ITERS = 40


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _input(kind):
    """(run, groups, stream, tables) of a named input; computed once, never changed"""
    run = {"standard": cc.standard_run, "tagged": lambda: cc.tagged(cc.standard_run()), "stopping": cc.stopping_run, "dedup": cc.dedup_run}[kind]()
    groups = dc.records_of(run)
    stream = dc.stream_of(groups)
    stream.setflags(write=False)
    return run, groups, stream, dc.tables_of(run)


@functools.lru_cache(maxsize=None)
def _model(kind, source="name", drop=False):
    run, groups, stream, tb = _input(kind)
    bcs, cnt = cc.barcodes_of(groups, source)
    dropped = cc.dropped_flags(len(run)) if drop else None
    name_cls, classes = cc.classes_of(groups, dropped)
    return bcs, cnt, name_cls, cc.model_of(bcs, name_cls, classes, cc.TX_FEATURE)


@functools.lru_cache(maxsize=None)
def _want(kind, mode, source="name", drop=False):
    return cc.matrix_of(_model(kind, source, drop)[3], mode)


@functools.lru_cache(maxsize=None)
def _spread(kind, mode, iters):
    return cc.spread_of(_model(kind)[3], mode, iters)


def _cuts(n, calls):
    return [0, n] if calls == 1 else [0, n // 3, n // 3 + 1, n]   # (a call of one name among them)


def _fill(objs, tb, stream, how):
    """the read names into the Quant / Cells / Dedup objects, call by call, from host memory or from HBM"""
    import torch
    go = tb["group_off"]
    cuts = _cuts(len(go) - 1, 3 if how.endswith("3") else 1)
    rec_off = lib.Sorter.row_offsets(stream)
    if how.startswith("dev"):
        t = [torch.from_numpy(x).cuda() for x in (tb["a"].view(np.int32), tb["cigar"].view(np.int64), tb["pool"].view(np.int32),
                                                  tb["row_off"].view(np.int64), go.view(np.int32), np.array(stream, dtype=np.uint8), rec_off.view(np.int64))]
        recs = lib.BrDeviceBam(t[5].data_ptr() if t[5].numel() else None, t[5].numel(), t[6].data_ptr(), t[6].numel() - 1)
    for g0, g1 in zip(cuts, cuts[1:]):
        for o in objs:
            if how.startswith("host"):
                if isinstance(o, lib.Quant):
                    o.add_host(tb["a"], tb["row_off"], go[g0:g1 + 1])
                elif isinstance(o, lib.Cells):
                    o.add_host(tb["row_off"], go[g0:g1 + 1], stream, rec_off)
                else:
                    o.add_host(tb["a"], tb["cigar"], tb["pool"], tb["row_off"], go[g0:g1 + 1], stream, rec_off)
            elif isinstance(o, lib.Quant):
                o.add_device(t[0], t[3], t[4], g0, g1)
            elif isinstance(o, lib.Cells):
                o.add_device(t[3], t[4], recs, g0, g1)
            else:
                o.add_device(t[0], t[1], t[2], t[3], t[4], recs, g0, g1)
    if how.startswith("dev"):
        torch.cuda.synchronize()


def _run(kind, how="dev1", drop=False, finish=True, **params):
    """-> (the Cells after finish, the Quant)"""
    run, groups, stream, tb = _input(kind)
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(**params)
    _fill((q, c), tb, stream, how)
    if drop:
        q.drop_names(cc.dropped_flags(len(run)))
    q.finish()
    if finish:
        c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    return c, q


def _assert_structure(c, kind, mode, source, drop, tag):
    """everything but the float values, bit for bit -> the device's values"""
    bcs, cnt, name_cls, model = _model(kind, source, drop)
    want = _want(kind, mode, source, drop) if mode == "unique" else cc.matrix_of(model, mode, 1, 0.0)   # (the structure needs no iteration)
    n = len(bcs)
    cb, ln = c.barcodes(0, n)
    wcb, wln = cc.barcode_matrix(bcs)
    assert np.array_equal(ln, wln) and np.array_equal(cb, wcb), tag
    assert (c.n_cells, c.n_entries) == (len(model["cells"]), len(want["feature"])), tag
    assert c.cell_barcodes() == model["cells"], tag
    assert np.array_equal(c.name_cells(0, n), model["name_cell"]), tag
    off, feat, val = c.matrix()
    assert off.dtype == np.uint64 and feat.dtype == np.uint32 and val.dtype == np.float64
    assert np.array_equal(off, want["off"]) and np.array_equal(feat, want["feature"]), tag
    cs = c.cell_stats()
    for k in ("names", "unique", "multi", "features"):
        assert np.array_equal(cs[k], want[k]), (tag, k)
    st = c.stats()
    assert (st["names"], st["no_barcode"], st["barcode_too_long"], st["bad_aux"]) == (n, cnt["no_barcode"], cnt["too_long"], cnt["bad_aux"]), tag
    assert st["counted"] == int(np.count_nonzero(model["name_cell"] != cc.NONE)) == int(want["names"].sum()), tag
    assert st["cells"] == len(model["cells"]) and st["entries"] == sum(len(e) for e in model["entries"]) and st["slots"] == sum(len(s) for s in model["slots"])
    assert st["pairs"] == sum(len(fs) for es in model["entries"] for _, _, fs in es)
    # a window of cells
    off2, feat2, val2 = c.matrix(3, 20)
    assert np.array_equal(off2, want["off"][3:24] - want["off"][3]) and np.array_equal(feat2, want["feature"][int(want["off"][3]):int(want["off"][23])])
    assert np.array_equal(val2.view(np.uint64), val[int(off[3]):int(off[23])].view(np.uint64))
    return val, cs, st


def _assert_values(got, ref, s, tag):
    print("%s: spread s of the restatement over three summation orders = %.3e" % (tag, s))
    assert 0 < s < 1e-9
    m = ref > 1e-6
    rel = float(np.max(np.abs(got[m] - ref[m]) / ref[m]))
    ab = float(np.max(np.abs(got[~m] - ref[~m]))) if (~m).any() else 0.0
    print("%s: device against the forward restatement: relative %.3e (bound %.3e), absolute below 1e-6 %.3e (bound %.3e)" % (tag, rel, 64 * s, ab, 64 * s * 1e-6))
    assert rel <= 64 * s and ab <= 64 * s * 1e-6


# ---- structure and the integer mode ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", HOWS)
def test_unique_matches_the_restatement_whatever_the_way_in(how):
    c, q = _run("standard", how, mode=0)
    val, cs, st = _assert_structure(c, "standard", "unique", "name", False, how)
    assert np.array_equal(val, _want("standard", "unique")["value"])
    assert not cs["iterations"].any() and (st["wave_cells"], st["block_cells"], st["hbm_cells"]) == (0, 0, 0)
    n = len(_input("standard")[0])
    assert c._raw("name_cells", 0, n + 1, None) == INVALID and c._raw("barcodes", -1, 1, None, None) == INVALID
    assert c._raw("cell_barcodes", c.n_cells, 1, None, None) == INVALID and c._raw("cell_barcodes", c.n_cells, 0, None, None) == 0
    c.close(), q.close()


@pytest.mark.parametrize("bits", [64, 4, 1])
def test_hash_width_and_dropped_names(bits):
    """the quantifier's classes collide at few bits and a tenth of the names is dropped: neither is the cells' business"""
    run, groups, stream, tb = _input("standard")
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    q.set_param("hash_bits", bits)
    c = lib.Cells(mode=0, hash_bits=bits)
    _fill((q, c), tb, stream, "dev3")
    q.drop_names(cc.dropped_flags(len(run)))
    q.finish()
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    val, _, _ = _assert_structure(c, "standard", "unique", "name", True, bits)
    assert np.array_equal(val, _want("standard", "unique", "name", True)["value"])
    assert int(_want("standard", "unique", "name", True)["names"].sum()) < int(_want("standard", "unique")["names"].sum())
    c.close(), q.close()


def test_the_tag_source_and_a_truncated_aux_field():
    for how in ("host3", "dev1"):
        c, q = _run("tagged", how, mode=0, barcode_source=1)
        val, _, st = _assert_structure(c, "tagged", "unique", "tag", False, how)
        assert st["bad_aux"] == 1 and np.array_equal(val, _want("tagged", "unique", "tag")["value"])
        c.close(), q.close()


def test_separator_and_tag_parameters():
    run = [dc.name_row(b"a:AAC:x", [(0, 5, dc.cig("30M"), 0)], b"XYZ" + b"GGT\0"), dc.name_row(b"b:AAC:y", [(2, 5, dc.cig("30M"), 0)], b"XYZ" + b"GG\0"),
           dc.name_row(b"c_AAG_z", [(0, 5, dc.cig("30M"), 0)], b"CBZ" + b"GGA\0")]
    groups = dc.records_of(run)
    stream, tb = dc.stream_of(groups), dc.tables_of(run)
    name_cls, classes = cc.classes_of(groups)
    for source, params, kw in (("name", {"barcode_sep": ":"}, {"sep": b":"}), ("tag", {"barcode_tag": "XY"}, {"tag": b"XY"})):
        bcs, _ = cc.barcodes_of(groups, source, **kw)
        model = cc.model_of(bcs, name_cls, classes, cc.TX_FEATURE)
        q = lib.Quant(cc.N_TX)
        q.set_param("keep_names", 1)
        c = lib.Cells(mode=0, barcode_source=cc.SOURCES[source], **params)
        _fill((q, c), tb, stream, "host")
        q.finish()
        c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
        assert c.cell_barcodes() == model["cells"] and np.array_equal(c.name_cells(0, 3), model["name_cell"]), source
        assert np.array_equal(c.matrix()[2], cc.matrix_of(model, "unique")["value"])
        c.close(), q.close()


# ---- the float modes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,iters", [("uniform", 1), ("em", EM_ITERS)])
def test_values_whatever_the_route(mode, iters):
    ref, s = _spread("standard", mode, iters)
    results = []
    for how, lds in (("dev1", None), ("dev3", None), ("host", None), ("dev1", cc.LDS_LOW), ("dev1", 0)):
        params = {"mode": cc.MODES[mode], "max_iters": iters, "tolerance": 0.0}
        if lds is not None:
            params["lds_bytes"] = lds
        c, q = _run("standard", how, **params)
        val, cs, st = _assert_structure(c, "standard", mode, "name", False, (mode, how, lds))
        assert np.array_equal(cs["iterations"], ref["iterations"]), (how, lds)
        assert st["wave_cells"] + st["block_cells"] + st["hbm_cells"] == st["cells"] and st["wave_cells"] > 50
        if lds is None:
            assert st["block_cells"] >= 4 and st["hbm_cells"] == 0
        elif lds:
            assert st["block_cells"] >= 1 and st["hbm_cells"] >= 1
        else:
            assert st["block_cells"] == 0 and st["hbm_cells"] >= 4
        _assert_values(val, ref["value"], s, "%s %s lds_bytes=%s" % (mode, how, lds))
        results.append(val)
        c.close(), q.close()
    # two runs, 1-call against 3-call adds, host against device tables: the same bits; the routes: the same code on other memory
    for other in results[1:]:
        assert np.array_equal(results[0].view(np.uint64), other.view(np.uint64))


def test_em_stops_where_the_restatement_stops():
    want = _want("stopping", "em")
    assert len(set(want["iterations"].tolist())) >= 5
    for lds in (None, 0):
        c, q = _run("stopping", "dev1", mode=2, **({} if lds is None else {"lds_bytes": lds}))
        off, feat, val = c.matrix()
        cs = c.cell_stats()
        bad = np.flatnonzero(cs["iterations"] != want["iterations"])
        assert bad.size == 0, (bad[:5], cs["iterations"][bad[:5]], want["iterations"][bad[:5]])
        assert np.array_equal(off, want["off"]) and np.array_equal(feat, want["feature"])
        assert np.allclose(val, want["value"], rtol=1e-9, atol=0)
        c.close(), q.close()
    c, q = _run("stopping", "dev1", mode=2, max_iters=3)   # the bound holds whatever the tolerance says
    assert np.array_equal(c.cell_stats()["iterations"], np.minimum(want["iterations"], 3))
    c.close(), q.close()


# ---- br_dedup per cell -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 4, 1])
@pytest.mark.parametrize("method", ["directional", "unique"])
def test_dedup_per_cell(method, bits):
    run, groups, stream, tb = _input("dedup")
    umis, _ = dc.umis_of(groups)
    bcs, _ = cc.barcodes_of(groups)
    rep, gf = cc.per_cell_molecules(method, groups, umis, bcs)
    for how in (("host3", "dev1") if bits == 64 else ("dev3",)):
        d = lib.Dedup(method=dc.METHODS[method], cell_source=1)
        _fill((d,), tb, stream, how)
        d.set_param("hash_bits", bits)
        assert d.finish() == dc.counts_of(rep), (method, bits, how)
        got_rep, got_gf, got_dup = d.result()
        for got, exp, what in ((got_gf, gf, "group_first"), (got_rep, rep, "rep"), (got_dup, dc.dup_of(rep), "dup")):
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (method, bits, how, what, bad[:5], got[bad[:5]], exp[bad[:5]])
        assert np.array_equal(d.hist(), dc.hist_of(rep))
        st = d.stats()
        assert st["groups"] == len(set(gf.tolist()) - {dc.NONE}) and (st["collisions"] > 0) == (bits < 64)
        d.close()
    # the head of the run: the same UMI and signature in two cells are two molecules, inside one cell one
    assert rep[0] == rep[2] == 0 and rep[1] != 0


def test_dedup_tag_cells_and_no_cell_source():
    run, groups, stream, tb = _input("tagged")
    umis, _ = dc.umis_of(groups)
    bcs, _ = cc.barcodes_of(groups, "tag")
    rep, gf = cc.per_cell_molecules("directional", groups, umis, bcs)
    d = lib.Dedup(cell_source=2, cell_tag="CB")
    _fill((d,), tb, stream, "dev1")
    d.finish()
    assert np.array_equal(d.result()[0], rep) and np.array_equal(d.result()[1], gf)
    d.close()
    # "cell_source" 0 is an object that never heard of the parameter
    run, groups, stream, tb = _input("dedup")
    res = []
    for params in ({}, {"cell_source": 0}):
        d = lib.Dedup(**params)
        _fill((d,), tb, stream, "dev3")
        counts = d.finish()
        st = d.stats()
        res.append((counts, d.result(), d.hist(), d.umis(0, len(run)), {k: st[k] for k in ("groups", "nodes", "edges", "sweeps", "max_group_nodes", "peak_bytes")}))
        d.close()
    assert res[0][0] == res[1][0] and res[0][4] == res[1][4]
    for a, b in zip(res[0][1] + (res[0][2],) + res[0][3], res[1][1] + (res[1][2],) + res[1][3]):
        assert np.array_equal(a, b)
    plain = dc.molecules_of("directional", dc.signatures_of(groups), dc.umis_of(groups)[0])
    assert np.array_equal(res[0][1][0], plain)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_errors():
    run, groups, stream, tb = _input("standard")
    # finish before the quantifier's, and without "keep_names"
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells()
    _fill((q, c), tb, stream, "host")
    assert c.finish_raw(q, cc.TX_FEATURE, cc.N_FEATURES) == INVALID
    assert c._raw("set_param", b"mode", 1) == INVALID and c._raw("set_tolerance", 0.5) == INVALID   # after the first add
    q.finish()
    q2 = lib.Quant(cc.N_TX)
    _fill((q2,), tb, stream, "host")
    q2.finish()
    assert c.finish_raw(q2, cc.TX_FEATURE, cc.N_FEATURES) == INVALID
    assert c.finish_raw(None, cc.TX_FEATURE, cc.N_FEATURES) == INVALID
    # a feature out of range
    bad = cc.TX_FEATURE.copy()
    bad[17] = cc.N_FEATURES
    assert c.finish_raw(q, bad, cc.N_FEATURES) == INVALID
    assert c._raw("matrix", 0, 0, None, None, None) == INVALID   # nothing has finished
    # a name-count mismatch
    c2 = lib.Cells()
    go = tb["group_off"]
    c2.add_host(tb["row_off"], go[:len(go) - 1], stream)
    assert c2.finish_raw(q, cc.TX_FEATURE, cc.N_FEATURES) == INVALID
    c2.close()
    # and every refusal left the object as it was
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    assert np.array_equal(c.matrix()[2], _want("standard", "unique")["value"])
    assert c.finish_raw(q, cc.TX_FEATURE, cc.N_FEATURES) == INVALID   # twice
    c.close(), q.close(), q2.close()
    # parameters out of range; descending offsets add nothing
    c = lib.Cells()
    for name, v in (("mode", 3), ("barcode_source", 2), ("lds_bytes", 65537), ("max_iters", 0), ("hash_bits", 0), ("nothing", 1)):
        assert c._raw("set_param", name.encode(), v) == INVALID, name
    assert c._raw("set_tolerance", -1.0) == INVALID
    ro = tb["row_off"].copy()
    ro[3] = ro[4] + 1
    rec_off = lib.Sorter.row_offsets(stream)
    data = np.array(stream)
    recs = lib.BrDeviceBam(data.ctypes.data, data.size, rec_off.ctypes.data, len(rec_off) - 1)
    assert c.add_raw(recs, ro.ctypes.data, len(rec_off) - 1, tb["group_off"].ctypes.data, len(tb["group_off"]) - 1, False) == INVALID
    assert c.add_raw(recs, tb["row_off"].ctypes.data, len(rec_off) - 2, tb["group_off"].ctypes.data, len(tb["group_off"]) - 1, False) == INVALID
    assert c.stats()["names"] == 0
    d = lib.Dedup()
    assert d._raw("set_param", b"cell_source", 3) == INVALID
    _fill((d,), tb, stream, "host")
    assert d._raw("set_param", b"cell_source", 1) == INVALID   # after the first add
    d.close()
    c.close()


def test_no_names_and_no_cells():
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    q.finish()
    c = lib.Cells(mode=2)
    assert c.finish(q, cc.TX_FEATURE, cc.N_FEATURES) == (0, 0)
    off, feat, val = c.matrix()
    assert list(off) == [0] and feat.size == 0 and val.size == 0 and c.cell_barcodes() == []
    c.close(), q.close()
    run = [dc.name_row(b"plain", [(0, 5, dc.cig("30M"), 0)]), dc.name_row(b"x_AC_T", [])]   # names, none of them counted
    groups = dc.records_of(run)
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(mode=2)
    _fill((q, c), dc.tables_of(run), dc.stream_of(groups), "host")
    q.finish()
    assert c.finish(q, cc.TX_FEATURE, cc.N_FEATURES) == (0, 0) and list(c.name_cells(0, 2)) == [cc.NONE] * 2
    c.close(), q.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
LINE = re.compile(r"\[bramble\] cells: (\d+) cells, (\d+) of (\d+) read names counted \((\d+) without barcode; (\d+) matrix entries; "
                  r"features (gene|transcript); multi (unique|uniform|em); add \d+\.\d\ds, finish \d+\.\d\ds\)$")


@functools.lru_cache(maxsize=None)
def _cli_input():
    """(annotation dict, the framed records of a synthetic paired input through with_cells_records, the transcript -> gene lines)"""
    from tests.test_gpu_collate import _inputs
    annd, recs, _ = _inputs("pe")
    ids = [tx["id"] for tx in annd["transcripts"]]
    gene_map = {t: "gene%d" % (i // 2) for i, t in enumerate(ids)}   # two transcripts a gene
    return annd, tuple(cc.with_cells_records(recs[:1200])), gene_map


def _cli_files(tmp_path):
    from tests import bamio
    from tests.test_gpu_collate import _cat, _files
    annd, recs, gene_map = _cli_input()
    gtf, tsv = str(tmp_path / "g.gtf"), str(tmp_path / "tx2gene.tsv")
    bamio.write_gtf(gtf, annd)
    open(tsv, "w").write("".join("%s\t%s\n" % kv for kv in gene_map.items()))
    bam, _ = _files(tmp_path, annd, _cat(list(recs)), "in")
    return bam, gtf, tsv


def _parse_cells(prefix):
    mtx = open(prefix + "matrix.mtx").read().split("\n")
    assert mtx[0].startswith("%%MatrixMarket matrix coordinate ") and mtx[0].endswith(" general") and mtx[-1] == ""
    kind = mtx[0].split()[3]
    body = [l.split() for l in mtx[1:-1] if not l.startswith("%")]
    dims = tuple(int(x) for x in body[0])
    rows = [(int(f), int(c), (int(v) if kind == "integer" else float(v)), v) for f, c, v in body[1:]]
    barcodes = open(prefix + "barcodes.tsv").read().split("\n")[:-1]
    features = [l.split("\t") for l in open(prefix + "features.tsv").read().split("\n")[:-1]]
    table = [l.split("\t") for l in open(prefix + "cells.tsv").read().split("\n")[:-1]]
    return kind, dims, rows, barcodes, features, table


@pytest.mark.parametrize("mode", ["unique", "uniform", "em"])
def test_cli_cells_with_dedup(tmp_path, mode):
    from tests import bamio
    from tests.test_gpu_collate import _report, _run, _strip
    bam, gtf, tsv = _cli_files(tmp_path)
    gene_map = _cli_input()[2]
    base = [bam, "-G", gtf, "--dedup", "directional", "--quant"]
    plain = _run(base + [str(tmp_path / "q0.tsv")], str(tmp_path / "o0.bam"))
    prefix = str(tmp_path / "c.")
    r = _run(base + [str(tmp_path / "q1.tsv"), "--cells", prefix, "--cells-multi", mode, "--quant-gene-map", tsv], str(tmp_path / "o1.bam"))
    t0, refs0, s0 = bamio.read_bam(str(tmp_path / "o0.bam"))
    t1, refs1, s1 = bamio.read_bam(str(tmp_path / "o1.bam"))
    assert _strip(t1) == _strip(t0) and refs1 == refs0 and np.array_equal(s1, s0)   # the main output
    assert _report(r) == _report(plain)                                              # and the final report
    # the restatement, fed from the run's own output
    groups = [g for _, g in dc.name_groups(s1)]
    assert len(groups) > 300
    umis, _ = dc.umis_of(groups)
    bcs, cnt = cc.barcodes_of(groups)
    rep, _ = cc.per_cell_molecules("directional", groups, umis, bcs)
    dup = dc.dup_of(rep)
    assert dup.sum() > 0.2 * len(dup) and not np.array_equal(rep, dc.molecules_of("directional", dc.signatures_of(groups), umis))
    name_cls, classes = cc.classes_of(groups, dup)
    genes = []
    for name, _ in refs1:
        if gene_map[name] not in genes:
            genes.append(gene_map[name])
    tx_feature = np.asarray([genes.index(gene_map[name]) for name, _ in refs1], np.uint32)
    model = cc.model_of(bcs, name_cls, classes, tx_feature)
    want = cc.matrix_of(model, mode)
    assert want["multi"].sum() > 0 and len(model["cells"]) == 12
    kind, dims, rows, barcodes, features, table = _parse_cells(prefix)
    assert kind == ("integer" if mode == "unique" else "real") and dims == (len(genes), len(model["cells"]), len(want["feature"]))
    assert barcodes == [b.decode() for b in model["cells"]]
    assert features == [[g, g, "Gene Expression"] for g in genes]
    cell_of = np.repeat(np.arange(len(model["cells"])), np.diff(want["off"].astype(np.int64)))
    assert [(f, c) for f, c, _, _ in rows] == [(int(f) + 1, int(c) + 1) for f, c in zip(want["feature"], cell_of)]   # by cell, then feature
    got = np.asarray([v for _, _, v, _ in rows], np.float64)
    if mode == "em":   # ten significant digits are printed
        assert np.allclose(got, want["value"], rtol=1e-9, atol=0)
    else:
        assert [text for _, _, _, text in rows] == [("%d" % v) if mode == "unique" else ("%.10g" % v) for v in want["value"]]
    assert table[0] == ["Barcode", "Names", "Unique", "Multi", "Features", "Iterations"]
    assert table[1:] == [[b.decode()] + [str(int(want[k][i])) for k in ("names", "unique", "multi", "features", "iterations")] for i, b in enumerate(model["cells"])]
    line = [l for l in r.stdout.decode().split("\n") if l.startswith("[bramble] cells:")]
    assert len(line) == 1 and LINE.match(line[0]), line
    m = LINE.match(line[0])
    assert (int(m.group(1)), int(m.group(2)), int(m.group(5)), m.group(6), m.group(7)) == (len(model["cells"]), int(want["names"].sum()), len(want["feature"]), "gene", mode)
    assert int(m.group(4)) >= cnt["no_barcode"] > 0 and int(m.group(3)) >= len(groups)
    # quant.tsv holds the per-cell molecules now
    assert open(str(tmp_path / "q1.tsv")).read() != open(str(tmp_path / "q0.tsv")).read()


def test_cli_cells_without_dedup_changes_no_other_output(tmp_path):
    from tests import bamio
    from tests.test_gpu_collate import _report, _run, _strip
    bam, gtf, tsv = _cli_files(tmp_path)
    plain = _run([bam, "-G", gtf, "--quant", str(tmp_path / "q0.tsv")], str(tmp_path / "o0.bam"))
    prefix = str(tmp_path / "t.")
    r = _run([bam, "-G", gtf, "--quant", str(tmp_path / "q1.tsv"), "--cells", prefix, "--cells-features", "transcript"], str(tmp_path / "o1.bam"))
    t0, refs0, s0 = bamio.read_bam(str(tmp_path / "o0.bam"))
    t1, refs1, s1 = bamio.read_bam(str(tmp_path / "o1.bam"))
    assert _strip(t1) == _strip(t0) and refs1 == refs0 and np.array_equal(s1, s0) and _report(r) == _report(plain)
    assert open(str(tmp_path / "q1.tsv")).read() == open(str(tmp_path / "q0.tsv")).read()
    groups = [g for _, g in dc.name_groups(s1)]
    bcs, _ = cc.barcodes_of(groups)
    name_cls, classes = cc.classes_of(groups)   # the unit is the read name
    model = cc.model_of(bcs, name_cls, classes, np.arange(len(refs1), dtype=np.uint32))
    want = cc.matrix_of(model, "unique")
    kind, dims, rows, barcodes, features, table = _parse_cells(prefix)
    assert kind == "integer" and dims == (len(refs1), len(model["cells"]), len(want["feature"]))
    assert features == [[n, n, "Gene Expression"] for n, _ in refs1]
    assert [(f - 1, v) for f, _, v, _ in rows] == [(int(f), int(v)) for f, v in zip(want["feature"], want["value"])]
    assert [int(t[1]) for t in table[1:]] == [int(x) for x in want["names"]]
    assert sorted(os.listdir(str(tmp_path))) == sorted(["g.gtf", "tx2gene.tsv", "in.bam", "q0.tsv", "q1.tsv", "o0.bam", "o1.bam"] + ["t." + x for x in ("matrix.mtx", "barcodes.tsv", "features.tsv", "cells.tsv")])


@pytest.mark.parametrize("extra,word", [
    (["--cells", "c."], b"--cells needs --quant"),
    (["--quant", "q.tsv", "--cells", "c.", "--devices", "0,1"], b"--cells works on one device"),
    (["--cells-multi", "em"], b"need --cells"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-multi", "most"], b"--cells-multi: unknown mode"),
])
def test_cli_refusals(tmp_path, extra, word):
    import subprocess
    from tests.test_gpu_collate import BIN
    r = subprocess.run([BIN, "in.bam", "-G", "g.gtf", "-o", "o.bam"] + extra, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr[:300]
    assert os.listdir(str(tmp_path)) == []


def test_cli_refuses_before_anything_is_projected(tmp_path):
    """gene features without a gene for every transcript, and a prefix whose directory is not there"""
    from tests.test_gpu_collate import _run
    bam, gtf, tsv = _cli_files(tmp_path)
    lines = open(tsv).read().split("\n")
    open(tsv, "w").write("\n".join(lines[1:]))   # the first transcript has no gene now
    r = _run([bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--cells", str(tmp_path / "c."), "--quant-gene-map", tsv], str(tmp_path / "o.bam"), ok=False)
    assert r.returncode != 0 and b"has no gene in it" in r.stderr and b"processing alignments" not in r.stdout
    r = _run([bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--cells", str(tmp_path / "nowhere" / "c.")], str(tmp_path / "o.bam"), ok=False)
    assert r.returncode != 0 and b"the directory of the prefix must exist" in r.stderr and b"processing alignments" not in r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["g.gtf", "in.bam", "tx2gene.tsv"]

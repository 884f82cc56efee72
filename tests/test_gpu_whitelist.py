"""The cell barcode whitelist on the GPU: br_whitelist's build and match, and br_cells, br_dedup and the command line with a whitelist
set, bit for bit against the tests' restatement of the definitions (tests/whitelist_cases.py: a brute-force Hamming search;
tests/test_whitelist_cpu.py pins it on the CPU and checks that the inputs used here reach every branch)."""
import functools
import os
import re

import numpy as np
import pytest

from bramble_amd import lib
from tests import cells_cases as cc
from tests import dedup_cases as dc
from tests import whitelist_cases as wc

pytestmark = pytest.mark.gpu

INVALID = -1
MODES = ("exact", "1mm", "1mm-multi")


def _assert_match(w, whitelist, observed, tag, modes=(0, 1, 2)):
    for correct in modes:
        want_e, want_s, _ = wc.resolve(whitelist, observed, correct)
        entry, status = w.match(list(observed), correct)
        bad = np.flatnonzero((entry != want_e) | (status != want_s))
        assert bad.size == 0, (tag, correct, bad[:5], [observed[i] for i in bad[:5]], entry[bad[:5]], want_e[bad[:5]], status[bad[:5]], want_s[bad[:5]])


# ---- build -------------------------------------------------------------------------------------------------------------------------
def _build_lists():
    rng = np.random.default_rng(11)
    mixed = [bytes(rng.choice(cc.ACGT, size=1 + k % 32).tolist()) for k in range(200)]   # lengths 1 .. 32
    base = wc.random_barcodes(rng, 1, 32)[0]
    edges = [base] + [dc.mutate(base, p) for p in wc.WORD_EDGES]                          # pairs that differ in one byte of a word's end
    short = [base[:p + 1] for p in wc.WORD_EDGES]
    return {"one": [b"ACGT"], "two": [b"TT", b"A"], "65": wc.far_whitelist(rng, 65, 10), "1000": wc.random_barcodes(rng, 1000, 14),
            "duplicates": [b"ACGT", b"AC", b"ACGT", b"AC", b"ACGT", b"G"], "mixed": mixed + mixed[:50], "edges": edges + short + edges[3:5]}


@pytest.mark.parametrize("kind", ["one", "two", "65", "1000", "duplicates", "mixed", "edges"])
def test_build_and_hash_width(kind):
    barcodes = _build_lists()[kind]
    want = wc.entries_of(barcodes)
    rng = np.random.default_rng(5)
    observed = list(barcodes) + [e for b in want[:40] for e in wc.every_error(b)[::7]] + [None, b"ACGTN", want[0] + b"A" if len(want[0]) < 32 else want[0][:31]]
    observed = [observed[i] for i in rng.permutation(len(observed))][:2500]
    got = {}
    for bits in (64, 4, 1):
        w = lib.Whitelist(barcodes, hash_bits=bits)
        st = w.stats()
        assert (st["given"], st["distinct"], w.n) == (len(barcodes), len(want), len(want)), (kind, bits)
        assert st["slots"] >= max(64, 2 * len(want)) and st["slots"] & (st["slots"] - 1) == 0 and 1 <= st["longest_chain"] <= st["slots"]
        if bits == 1 and len(want) > 2:
            assert st["longest_chain"] >= len(want) // 2   # two home slots: the chains are walked
        assert w.barcodes() == want, (kind, bits)
        assert w.barcodes(len(want) // 2, len(want) - len(want) // 2) == want[len(want) // 2:]
        assert w._raw("barcodes", len(want), 1, None, None) == INVALID and w._raw("barcodes", len(want), 0, None, None) == 0
        _assert_match(w, barcodes, observed, (kind, bits))
        got[bits] = [w.match(observed, c) for c in (0, 1, 2)]
        w.close()
    for bits in (4, 1):
        for (e0, s0), (e1, s1) in zip(got[64], got[bits]):
            assert np.array_equal(e0, e1) and np.array_equal(s0, s1)


# ---- match -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, 8, 9, 16, 17, 32])
def test_every_error_at_every_position(length):
    """an error at every position with every base maps back to its entry; positions 15 / 16 are where a variant moves from a lane's
    first probe to its second"""
    rng = np.random.default_rng(length)
    whitelist = wc.far_whitelist(rng, 4 if length == 1 else 12, length) if length > 2 else [b"A"]
    observed = [e for b in whitelist for e in wc.every_error(b)] + list(whitelist)
    observed += [wc.put(b, p, ord("N")) for b in whitelist[:3] for p in range(length)]   # N at every position
    assert len(observed) >= 3 * length + 1
    for bits in (64, 1):
        w = lib.Whitelist(whitelist, hash_bits=bits)
        _assert_match(w, whitelist, observed, (length, bits))
        entry, status = w.match(observed, 1)
        if length > 2:
            assert (status[:3 * length * len(whitelist)] == wc.CORRECTED).all() and (entry != wc.NONE).all()
        w.close()


def test_the_branches():
    whitelist, observed = wc.branch_case()
    w = lib.Whitelist(whitelist)
    _assert_match(w, whitelist, observed, "branch")
    w.close()
    # by hand: an exact hit that lies one byte from another entry; two and three candidates; counts; a tie; candidates nobody carries;
    # a non-ACGT barcode that is itself an entry; distance two; the same prefix at another length
    wl = [b"AAAA", b"AAAC", b"AAAG", b"CCCC", b"GGGG", b"GGTT", b"TTTTT", b"ACGT", b"NNXN"]
    w = lib.Whitelist(wl)
    assert w.barcodes() == [b"AAAA", b"AAAC", b"AAAG", b"ACGT", b"CCCC", b"GGGG", b"GGTT", b"NNXN", b"TTTTT"]
    obs = [b"AAAA", b"AAAT", b"GGGT", b"GGGG", b"GGGG", b"GGTT", b"CCCA", b"NNXN", b"NNAA", b"CCAA", b"TTTT", b"TTTTTT", None, b"AAAC", b"AAAC", b"NCGT"]
    N = wc.NONE
    e, s = w.match(obs, 0)
    assert e.tolist() == [0, N, N, 5, 5, 6, N, 7, N, N, N, N, N, 1, 1, N] and s.tolist() == [1, 3, 3, 1, 1, 1, 3, 1, 3, 3, 3, 3, 0, 1, 1, 3]
    e, s = w.match(obs, 1)   # AAAT: three candidates; GGGT: two; CCCA and NCGT: one
    assert e.tolist() == [0, N, N, 5, 5, 6, 4, 7, N, N, N, N, N, 1, 1, 3] and s.tolist() == [1, 4, 4, 1, 1, 1, 2, 1, 3, 3, 3, 3, 0, 1, 1, 2]
    e, s = w.match(obs, 2)   # AAAT -> AAAC (2 > 1 > 0); GGGT -> GGGG (2 > 1); CCCA, NCGT: candidates of count 0
    assert e.tolist() == [0, 1, 5, 5, 5, 6, N, 7, N, N, N, N, N, 1, 1, N] and s.tolist() == [1, 2, 2, 1, 1, 1, 3, 1, 3, 3, 3, 3, 0, 1, 1, 3]
    e, s = w.match([b"AAAA", b"AAAC", b"AAAT"], 2)   # a tie on the largest count
    assert e.tolist() == [0, 1, N] and s.tolist() == [1, 1, 4]
    for ob in (obs, [b"AAAA", b"AAAC", b"AAAT"]):
        _assert_match(w, wl, ob, "hand")
    w.close()


@pytest.mark.parametrize("d", [0, 1, 63, 64, 65, 257])
def test_distinct_observed_at_wave_and_block_edges(d):
    """d distinct observed barcodes, all of them misses with one candidate, each carried by one to three names"""
    rng = np.random.default_rng(d)
    whitelist = wc.far_whitelist(rng, 300, 14)
    observed = [dc.mutate(b, k % 14) for k, b in enumerate(whitelist[:d]) for _ in range(1 + k % 3)]
    observed = [observed[i] for i in rng.permutation(len(observed))] + [None] * (d % 2)
    w = lib.Whitelist(whitelist, hash_bits=64 if d % 2 else 3)
    _assert_match(w, whitelist, observed, d)
    if d:
        assert (w.match(observed, 1)[1][:len(observed) - d % 2] == wc.CORRECTED).all()
    e, s = w.match([], 1)   # n = 0
    assert e.size == 0 and s.size == 0
    w.close()


# ---- br_cells ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _input():
    run, whitelist = wc.run_case()
    run = list(run)
    groups = dc.records_of(run)
    stream = dc.stream_of(groups)
    stream.setflags(write=False)
    return run, groups, stream, dc.tables_of(run), whitelist, tuple(wc.observed_of(groups))


def _fill(objs, tb, stream, cuts, device):
    """the read names into the Quant / Cells / Dedup objects, add by add (cuts: the adds' first names and the end), from host memory or HBM"""
    import torch
    go = tb["group_off"]
    rec_off = lib.Sorter.row_offsets(stream)
    if device:
        t = [torch.from_numpy(x).cuda() for x in (tb["a"].view(np.int32), tb["cigar"].view(np.int64), tb["pool"].view(np.int32),
                                                  tb["row_off"].view(np.int64), go.view(np.int32), np.array(stream, dtype=np.uint8), rec_off.view(np.int64))]
        recs = lib.BrDeviceBam(t[5].data_ptr() if t[5].numel() else None, t[5].numel(), t[6].data_ptr(), t[6].numel() - 1)
    for g0, g1 in zip(cuts, cuts[1:]):
        for o in objs:
            if not device:
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
    if device:
        torch.cuda.synchronize()


def _cuts(n, adds):
    return [0, n] if adds == 1 else [0, 3, n] if adds == 2 else [0, 2, 3, n // 2, n - 2, n]   # (name 2 is corrected by the last three)


def _cells(correct, adds=1, device=True, bits=64, **params):
    run, groups, stream, tb, whitelist, observed = _input()
    w = lib.Whitelist(whitelist, hash_bits=bits)
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(**params)
    c.set_whitelist(w, correct)
    _fill((q, c), tb, stream, _cuts(len(run), adds), device)
    q.finish()
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    return c, q, w


@pytest.mark.parametrize("correct", MODES)
def test_cells_with_a_whitelist(correct):
    run, groups, stream, tb, whitelist, observed = _input()
    entry, status, resolved = wc.resolve(whitelist, observed, wc.CORRECT[correct])
    name_cls, classes = cc.classes_of(groups)
    model = cc.model_of(resolved, name_cls, classes, cc.TX_FEATURE)
    want = cc.matrix_of(model, "unique")
    n = len(run)
    seen = []
    for adds, device, bits in ((1, True, 64), (2, False, 64), (5, True, 1), (5, False, 4)):
        c, q, w = _cells(correct, adds, device, bits, mode=0)
        tag = (correct, adds, device, bits)
        assert np.array_equal(c.name_status(0, n), status), tag
        cb, ln = c.barcodes(0, n)   # the resolved barcodes
        wcb, wln = cc.barcode_matrix(resolved)
        assert np.array_equal(ln, wln) and np.array_equal(cb, wcb), tag
        assert c.cell_barcodes() == model["cells"] and np.array_equal(c.name_cells(0, n), model["name_cell"]), tag
        assert set(model["cells"]) <= set(whitelist)
        off, feat, val = c.matrix()
        assert np.array_equal(off, want["off"]) and np.array_equal(feat, want["feature"]) and np.array_equal(val, want["value"]), tag
        cs = c.cell_stats()
        for k in ("names", "unique", "multi", "features"):
            assert np.array_equal(cs[k], want[k]), (tag, k)
        ws = c.whitelist_stats()
        counts = np.bincount(status, minlength=5)
        assert [ws[k] for k in ("no_barcode", "exact", "corrected", "no_match", "ambiguous")] == counts.tolist(), tag
        assert ws["distinct_observed"] == len({b for b in observed if b is not None}) and ws["correct"] == wc.CORRECT[correct]
        st = c.stats()   # the existing words keep their meaning: no_barcode is the add's count
        assert st["names"] == n and st["no_barcode"] == cc.barcodes_of(groups)[1]["no_barcode"] and st["counted"] == int(want["names"].sum())
        assert c._raw("name_status", 0, n + 1, None) == INVALID
        # Corrected: the counted names of the cell whose status is 2
        cell = c.name_cells(0, n)
        corrected = np.bincount(cell[(status == wc.CORRECTED) & (cell != cc.NONE)], minlength=len(model["cells"]))
        seen.append(corrected)
        c.close(), q.close(), w.close()
    if correct != "exact":
        assert seen[0].sum() > 0
    else:
        assert seen[0].sum() == 0
    for other in seen[1:]:
        assert np.array_equal(seen[0], other)


@pytest.mark.parametrize("mode,iters", [("uniform", 1), ("em", 40)])
def test_cells_values_with_a_whitelist(mode, iters):
    """the float modes over the resolved barcodes, under tests/test_gpu_cells.py's accuracy rule with the restatement's own spread"""
    from tests.test_gpu_cells import _assert_values
    run, whitelist = wc.values_case()
    run = list(run)
    groups = dc.records_of(run)
    stream, tb = dc.stream_of(groups), dc.tables_of(run)
    _, status, resolved = wc.resolve(whitelist, wc.observed_of(groups), 2)
    name_cls, classes = cc.classes_of(groups)
    model = cc.model_of(resolved, name_cls, classes, cc.TX_FEATURE)
    ref, s = cc.spread_of(model, mode, iters)
    w = lib.Whitelist(whitelist)
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(mode=cc.MODES[mode], max_iters=iters, tolerance=0.0)
    c.set_whitelist(w, "1mm-multi")
    _fill((q, c), tb, stream, [0, len(run) // 2, len(run)], True)
    q.finish()
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    assert np.array_equal(c.name_status(0, len(run)), status) and c.cell_barcodes() == model["cells"]
    off, feat, val = c.matrix()
    assert np.array_equal(off, ref["off"]) and np.array_equal(feat, ref["feature"])
    assert np.array_equal(c.cell_stats()["iterations"], ref["iterations"])
    _assert_values(val, ref["value"], s, "whitelist %s" % mode)
    c.close(), q.close(), w.close()


def test_cells_without_a_whitelist_are_as_before():
    run, groups, stream, tb, whitelist, observed = _input()
    name_cls, classes = cc.classes_of(groups)
    model = cc.model_of(list(observed), name_cls, classes, cc.TX_FEATURE)
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(mode=0)
    _fill((q, c), tb, stream, [0, len(run)], True)
    q.finish()
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    assert c.cell_barcodes() == model["cells"] and np.array_equal(c.name_cells(0, len(run)), model["name_cell"])
    assert np.array_equal(c.matrix()[2], cc.matrix_of(model, "unique")["value"])
    assert c._raw("name_status", 0, 1, None) == INVALID and c._raw("whitelist_stats", None) == INVALID
    assert len(model["cells"]) > len(cc.model_of(wc.resolve(whitelist, observed, 1)[2], name_cls, classes, cc.TX_FEATURE)["cells"])
    c.close(), q.close()


# ---- br_dedup ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["directional", "unique"])
@pytest.mark.parametrize("correct", ["1mm", "1mm-multi"])
def test_dedup_per_cell_with_a_whitelist(method, correct):
    run, groups, stream, tb, whitelist, observed = _input()
    umis, _ = dc.umis_of(groups)
    _, status, resolved = wc.resolve(whitelist, observed, wc.CORRECT[correct])
    rep, gf = cc.per_cell_molecules(method, groups, umis, resolved)
    plain, _ = cc.per_cell_molecules(method, groups, umis, list(observed))
    assert rep[1] == rep[0] == 0 and plain[1] == 1   # two copies, one with a barcode error: one molecule with the whitelist, two without
    for adds, device, bits in ((1, True, 64), (5, False, 1)):
        w = lib.Whitelist(whitelist, hash_bits=bits)
        d = lib.Dedup(method=dc.METHODS[method], cell_source=1)
        d.set_whitelist(w, correct)
        _fill((d,), tb, stream, _cuts(len(run), adds), device)
        assert d.finish() == dc.counts_of(rep), (method, correct, adds)
        got_rep, got_gf, got_dup = d.result()
        for got, exp, what in ((got_gf, gf, "group_first"), (got_rep, rep, "rep"), (got_dup, dc.dup_of(rep), "dup")):
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (method, correct, adds, what, bad[:5], got[bad[:5]], exp[bad[:5]])
        ws = d.whitelist_stats()
        assert [ws[k] for k in ("no_barcode", "exact", "corrected", "no_match", "ambiguous")] == np.bincount(status, minlength=5).tolist()
        d.close(), w.close()
    d = lib.Dedup(method=dc.METHODS[method], cell_source=1)   # the same input without the whitelist
    _fill((d,), tb, stream, [0, len(run)], True)
    d.finish()
    assert np.array_equal(d.result()[0], plain) and d.result()[0][1] == 1
    d.close()


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_errors():
    import torch
    run, groups, stream, tb, whitelist, observed = _input()
    cb, ln = lib.Whitelist.pack([b"ACGT", b"", b"AC"])
    assert lib.Whitelist.new_raw(0, cb, ln, 3) == (INVALID, None)            # a length of 0
    cb, ln = lib.Whitelist.pack([b"ACGT", b"A" * 33])
    assert lib.Whitelist.new_raw(0, cb, ln, 2) == (INVALID, None)            # of 33
    cb, ln = lib.Whitelist.pack([b"ACGT"])
    assert lib.Whitelist.new_raw(0, cb, ln, 0) == (INVALID, None)            # no barcode
    assert lib.Whitelist.new_raw(0, cb, ln, 1, hash_bits=65) == (INVALID, None)
    assert lib.Whitelist.new_raw(torch.cuda.device_count(), cb, ln, 1)[0] != 0 and lib.Whitelist.new_raw(0, cb, ln, 1)[0] == 0
    w = lib.Whitelist(whitelist)
    ocb, oln = lib.Whitelist.pack([b"ACGT", b"A" * 40])
    assert w.match_raw(ocb, oln, 2, 1)[0] == INVALID and w.match_raw(ocb, oln, 1, 3)[0] == INVALID and w.match_raw(ocb, oln, 1, -1)[0] == INVALID
    # a bad "correct"; no whitelist; after finish -- and the object is as it was: the finish below resolves under "1mm"
    q = lib.Quant(cc.N_TX)
    q.set_param("keep_names", 1)
    c = lib.Cells(mode=0)
    c.set_whitelist(w, "1mm")
    assert c._raw("set_whitelist", w.h, 3) == INVALID and c._raw("set_whitelist", w.h, -1) == INVALID and c._raw("set_whitelist", None, 1) == INVALID
    _fill((q, c), tb, stream, [0, len(run)], False)
    assert c.finish_raw(q, cc.TX_FEATURE, cc.N_FEATURES) == INVALID            # the quantifier has not finished: nothing was resolved
    assert c.barcodes(0, len(run))[1].tolist() == cc.barcode_matrix(list(observed))[1].tolist()
    assert np.array_equal(c.barcodes(0, len(run))[0], cc.barcode_matrix(list(observed))[0])
    q.finish()
    c.finish(q, cc.TX_FEATURE, cc.N_FEATURES)
    assert c._raw("set_whitelist", w.h, 0) == INVALID
    assert np.array_equal(c.name_status(0, len(run)), wc.resolve(whitelist, observed, 1)[1])
    c.close(), q.close()
    d = lib.Dedup()
    assert d._raw("set_whitelist", w.h, 1) == INVALID                          # without "cell_source"
    _fill((d,), tb, stream, [0, len(run)], False)
    d.finish()
    assert np.array_equal(d.result()[0], dc.molecules_of("directional", dc.signatures_of(groups), dc.umis_of(groups)[0]))
    d.close()
    d = lib.Dedup(cell_source=1)
    assert d._raw("set_whitelist", w.h, 3) == INVALID and d._raw("whitelist_stats", None) == INVALID
    _fill((d,), tb, stream, [0, len(run)], False)
    d.finish()
    assert d._raw("set_whitelist", w.h, 1) == INVALID                          # after finish
    assert np.array_equal(d.result()[0], cc.per_cell_molecules("directional", groups, dc.umis_of(groups)[0], list(observed))[0])
    d.close()
    if torch.cuda.device_count() > 1:                                          # another device's whitelist
        w1 = lib.Whitelist(whitelist, device=1)
        c, d = lib.Cells(), lib.Dedup(cell_source=1)
        assert c._raw("set_whitelist", w1.h, 1) == INVALID and d._raw("set_whitelist", w1.h, 1) == INVALID
        c.close(), d.close(), w1.close()
    w.close()


# ---- the command line ----------------------------------------------------------------------------------------------------------------
WL_LINE = re.compile(r"\[bramble\] whitelist: (\d+) barcodes; (\d+) read names with a barcode: (\d+) exact, (\d+) corrected, (\d+) without match, "
                     r"(\d+) ambiguous \((\d+) distinct observed; correct (exact|1mm|1mm-multi); build \d+\.\d\ds, resolve \d+\.\d\ds\)$")


@functools.lru_cache(maxsize=None)
def _cli_input():
    from tests.test_gpu_collate import _inputs
    annd, recs, _ = _inputs("pe")
    ids = [tx["id"] for tx in annd["transcripts"]]
    return annd, tuple(wc.with_barcode_errors(recs[:1200])), {t: "gene%d" % (i // 2) for i, t in enumerate(ids)}


def _cli_files(tmp_path):
    from tests import bamio
    from tests.test_gpu_collate import _cat, _files
    annd, recs, gene_map = _cli_input()
    gtf, tsv, txt = str(tmp_path / "g.gtf"), str(tmp_path / "tx2gene.tsv"), str(tmp_path / "wl.txt")
    bamio.write_gtf(gtf, annd)
    open(tsv, "w").write("".join("%s\t%s\n" % kv for kv in gene_map.items()))
    open(txt, "wb").write(b"# the cells\r\n" + b"".join(b + b"\t1\r\n" for b in wc.cli_whitelist()[1]) + b"\n")
    bam, _ = _files(tmp_path, annd, _cat(list(recs)), "in")
    return bam, gtf, tsv, txt


@pytest.mark.parametrize("dedup", [True, False])
@pytest.mark.parametrize("correct", MODES)
def test_cli_whitelist(tmp_path, correct, dedup):
    from tests import bamio
    from tests.test_gpu_cells import LINE, _parse_cells
    from tests.test_gpu_collate import _run
    bam, gtf, tsv, txt = _cli_files(tmp_path)
    gene_map = _cli_input()[2]
    prefix = str(tmp_path / "c.")
    args = [bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--cells", prefix, "--quant-gene-map", tsv, "--cells-whitelist", txt]
    args += (["--dedup", "directional"] if dedup else []) + (["--cells-correct", correct] if correct != "1mm" else [])   # (1mm is the default)
    r = _run(args, str(tmp_path / "o.bam"))
    _, refs, s = bamio.read_bam(str(tmp_path / "o.bam"))
    groups = [g for _, g in dc.name_groups(s)]
    observed = wc.observed_of(groups)
    whitelist = wc.cli_whitelist()[1]
    assert wc.reaches_every_branch(whitelist, observed) and 300 < len(groups) < 4000
    _, status, resolved = wc.resolve(whitelist, observed, wc.CORRECT[correct])
    dup = None
    if dedup:
        rep, _ = cc.per_cell_molecules("directional", groups, dc.umis_of(groups)[0], resolved)
        dup = dc.dup_of(rep)
        assert not np.array_equal(rep, cc.per_cell_molecules("directional", groups, dc.umis_of(groups)[0], observed)[0])
    name_cls, classes = cc.classes_of(groups, dup)
    genes = []
    for name, _ in refs:
        if gene_map[name] not in genes:
            genes.append(gene_map[name])
    tx_feature = np.asarray([genes.index(gene_map[name]) for name, _ in refs], np.uint32)
    model = cc.model_of(resolved, name_cls, classes, tx_feature)
    want = cc.matrix_of(model, "unique")
    kind, dims, rows, barcodes, features, table = _parse_cells(prefix)
    assert kind == "integer" and dims == (len(genes), len(model["cells"]), len(want["feature"]))
    assert barcodes == [b.decode() for b in model["cells"]] and set(model["cells"]) <= set(whitelist)   # the barcodes printed are entries
    assert features == [[g, g, "Gene Expression"] for g in genes]
    cell_of = np.repeat(np.arange(len(model["cells"])), np.diff(want["off"].astype(np.int64)))
    assert [(f, c, v) for f, c, v, _ in rows] == [(int(f) + 1, int(c) + 1, int(v)) for f, c, v in zip(want["feature"], cell_of, want["value"])]
    cell = model["name_cell"]
    corrected = np.bincount(cell[(status == wc.CORRECTED) & (cell != cc.NONE)], minlength=len(model["cells"]))
    assert table[0] == ["Barcode", "Names", "Unique", "Multi", "Features", "Iterations", "Corrected"]
    assert table[1:] == [[b.decode()] + [str(int(want[k][i])) for k in ("names", "unique", "multi", "features", "iterations")] + [str(int(corrected[i]))]
                         for i, b in enumerate(model["cells"])]
    assert (corrected.sum() > 0) == (correct != "exact")
    out = r.stdout.decode().split("\n")
    lines = [l for l in out if l.startswith("[bramble] whitelist:")]
    assert len(lines) == 1 and WL_LINE.match(lines[0]), lines
    m = WL_LINE.match(lines[0])
    counts = np.bincount(status, minlength=5)
    assert [int(m.group(k)) for k in range(1, 8)] == [len(whitelist), int(counts[1:].sum())] + counts[1:].tolist() + [len({b for b in observed if b is not None})]
    assert m.group(8) == correct
    cells_line = [i for i, l in enumerate(out) if LINE.match(l)]
    assert len(cells_line) == 1 and out.index(lines[0]) < cells_line[0]   # the cells: line keeps its text, behind the whitelist's
    assert len([l for l in out if l.startswith("[bramble] dedup:")]) == (1 if dedup else 0)


def test_cli_without_the_switch_is_as_before(tmp_path):
    from tests import bamio
    from tests.test_gpu_cells import _parse_cells
    from tests.test_gpu_collate import _run
    bam, gtf, tsv, txt = _cli_files(tmp_path)
    prefix = str(tmp_path / "t.")
    r = _run([bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--cells", prefix, "--cells-features", "transcript"], str(tmp_path / "o.bam"))
    _, refs, s = bamio.read_bam(str(tmp_path / "o.bam"))
    groups = [g for _, g in dc.name_groups(s)]
    name_cls, classes = cc.classes_of(groups)
    model = cc.model_of(wc.observed_of(groups), name_cls, classes, np.arange(len(refs), dtype=np.uint32))
    want = cc.matrix_of(model, "unique")
    kind, dims, rows, barcodes, features, table = _parse_cells(prefix)
    assert barcodes == [b.decode() for b in model["cells"]] and len(barcodes) > 3 * len(wc.cli_whitelist()[0])   # one cell per error
    assert table[0] == ["Barcode", "Names", "Unique", "Multi", "Features", "Iterations"]
    assert table[1:] == [[b.decode()] + [str(int(want[k][i])) for k in ("names", "unique", "multi", "features", "iterations")] for i, b in enumerate(model["cells"])]
    assert [(f - 1, v) for f, _, v, _ in rows] == [(int(f), int(v)) for f, v in zip(want["feature"], want["value"])]
    assert b"whitelist" not in r.stdout


@pytest.mark.parametrize("extra,word", [
    (["--quant", "q.tsv", "--cells-whitelist", "wl.txt"], b"--cells-whitelist needs --cells"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-correct", "1mm"], b"--cells-correct needs --cells-whitelist"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-whitelist", "wl.txt", "--cells-correct", "2mm"], b"--cells-correct: unknown mode"),
])
def test_cli_refusals(tmp_path, extra, word):
    import subprocess
    from tests.test_gpu_collate import BIN
    r = subprocess.run([BIN, "in.bam", "-G", "g.gtf", "-o", "o.bam"] + extra, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr[:300]
    assert os.listdir(str(tmp_path)) == []


def test_cli_refuses_a_bad_list_before_anything_is_projected(tmp_path):
    from tests.test_gpu_collate import _run
    bam, gtf, tsv, txt = _cli_files(tmp_path)
    base = [bam, "-G", gtf, "--quant", str(tmp_path / "q.tsv"), "--cells", str(tmp_path / "c."), "--quant-gene-map", tsv, "--cells-whitelist"]
    r = _run(base + [str(tmp_path / "nowhere.txt")], str(tmp_path / "o.bam"), ok=False)                  # an unreadable file
    assert r.returncode != 0 and b"nowhere.txt" in r.stderr and b"could not read" in r.stderr and b"processing alignments" not in r.stdout
    open(txt, "wb").write(b"ACGTACGT\n" + b"A" * 33 + b"\n")                                            # a 33-byte line
    r = _run(base + [txt], str(tmp_path / "o.bam"), ok=False)
    assert r.returncode != 0 and b"wl.txt line 2" in r.stderr and b"processing alignments" not in r.stdout
    assert sorted(os.listdir(str(tmp_path))) == ["g.gtf", "in.bam", "tx2gene.tsv", "wl.txt"]

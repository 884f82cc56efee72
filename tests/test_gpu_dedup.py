"""--dedup on the GPU: br_dedup's UMIs, verdicts (rep, group_first, dup), histogram, counts and record stream against the tests'
restatement of the definitions (tests/dedup_cases.py; tests/test_dedup_cpu.py pins it on the CPU and checks the inputs used here), bit
for bit: through every way in, both methods and UMI sources, at every hash width, on groups and names around the kernels' tiles, on
the chain that needs the most sweeps, with a regrowing arena; the errors; br_quant_drop_names against a quantifier that never saw the
duplicates."""
import functools
import os
import re

import numpy as np
import pytest

from bramble_amd import lib
from tests import dedup_cases as dc

pytestmark = pytest.mark.gpu

BIG = 1 << 30
INVALID, CAPACITY = -1, -5
HOWS = ("host", "host3", "dev1", "dev3")


# ---- helpers ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _input(kind, tag=False):
    """(run, groups, stream, tables) of a named input; computed once, never changed"""
    if kind == "standard":
        run = dc.standard_run(tag=tag)
    elif kind == "no-dups":
        run = [dc.name_row(b"solo%d_ACGTACGT" % i, [(i % 5, 100 + i, dc.cig("30M"), 0)]) for i in range(70)]
    elif kind == "one":
        run = [dc.name_row(b"only_ACGT", [(0, 10, dc.cig("4S26M"), 16)])]
    elif kind == "chain":
        run = dc.chain(96)
    elif kind == "paper":
        run = dc.paper_network()
    groups = dc.records_of(run, spill_every=7)
    stream = dc.stream_of(groups)
    stream.setflags(write=False)
    return run, groups, stream, dc.tables_of(run)


@functools.lru_cache(maxsize=None)
def _expected(kind, tag, method, source):
    run, groups, stream, tb = _input(kind, tag)
    umis, cnt = dc.umis_of(groups, source)
    sigs = dc.signatures_of(groups)
    rep = dc.molecules_of(method, sigs, umis)
    return {"umis": dc.umi_matrix(umis), "cnt": cnt, "gf": dc.groups_of(sigs), "rep": rep, "dup": dc.dup_of(rep), "hist": dc.hist_of(rep),
            "counts": dc.counts_of(rep)}


def _cuts(n, calls):
    return [0, n] if calls == 1 else [0, n // 3, n // 3 + 1, n]   # (a call of one name among them)


def _fill(d, tb, stream, how):
    """the read names into the Dedup, call by call, from host memory ("host", "host3") or from HBM ("dev1", "dev3")"""
    import torch
    go = tb["group_off"]
    cuts = _cuts(len(go) - 1, 3 if how.endswith("3") else 1)
    rec_off = lib.Sorter.row_offsets(stream)
    if how.startswith("dev"):
        t = [torch.from_numpy(x).cuda() for x in (tb["a"].view(np.int32), tb["cigar"].view(np.int64), tb["pool"].view(np.int32),
                                                  tb["row_off"].view(np.int64), go.view(np.int32), np.array(stream, dtype=np.uint8), rec_off.view(np.int64))]
        recs = lib.BrDeviceBam(t[5].data_ptr() if t[5].numel() else None, t[5].numel(), t[6].data_ptr(), t[6].numel() - 1)
    for g0, g1 in zip(cuts, cuts[1:]):
        if how.startswith("host"):
            d.add_host(tb["a"], tb["cigar"], tb["pool"], tb["row_off"], go[g0:g1 + 1], stream, rec_off)
        else:
            d.add_device(t[0], t[1], t[2], t[3], t[4], recs, g0, g1)
    if how.startswith("dev"):
        torch.cuda.synchronize()


def _assert_result(d, want, tag):
    n = len(want["rep"])
    assert d.finish() == want["counts"], tag
    umi, ln = d.umis(0, n)
    assert np.array_equal(ln, want["umis"][1]) and np.array_equal(umi, want["umis"][0]), tag
    rep, gf, dup = d.result()
    assert rep.dtype == np.uint32 and dup.dtype == np.uint8
    for got, exp, what in ((gf, want["gf"], "group_first"), (rep, want["rep"], "rep"), (dup, want["dup"], "dup")):
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (tag, what, bad[:5], got[bad[:5]], exp[bad[:5]])
    assert np.array_equal(d.hist(), want["hist"]), tag
    st = d.stats()
    assert (st["names"], st["no_umi"], st["umi_too_long"], st["bad_aux"]) == (n, want["cnt"]["no_umi"], want["cnt"]["too_long"], want["cnt"]["bad_aux"]), tag
    assert st["groups"] == len(set(want["gf"].tolist()) - {dc.NONE}) and st["names_with_rows"] == int(np.count_nonzero(want["rep"] != dc.NONE))
    return st


def _drain(d, max_bytes):
    parts, sizes = [], []
    for data, off in d.pieces(max_bytes):
        assert off[0] == 0 and int(off[-1]) == data.size and np.all(np.diff(off) > 0)
        parts.append(data)
        sizes.append((int(data.size), len(off) - 1))
    assert d.next_records(max_bytes).n_rows == 0   # a draw after the last
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), sizes


# ---- verdicts --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["name", "tag"])
@pytest.mark.parametrize("method", ["directional", "unique"])
def test_verdicts_match_the_restatement_whatever_the_way_in(method, source):
    tag = source == "tag"
    run, groups, stream, tb = _input("standard", tag)
    want = _expected("standard", tag, method, source)
    assert want["counts"][2] > 0.3 * want["counts"][0]
    for how in HOWS:
        d = lib.Dedup(method=dc.METHODS[method], umi_source=dc.SOURCES[source])
        _fill(d, tb, stream, how)
        st = _assert_result(d, want, (method, source, how))
        assert st["collisions"] == 0 and st["max_group_nodes"] == 257
        assert (st["edges"] > 0 and st["sweeps"] >= 95) if method == "directional" and not tag else True
        rep2, gf2, dup2 = d.result(5, 40)   # a window
        assert np.array_equal(rep2, want["rep"][5:45]) and np.array_equal(dup2, want["dup"][5:45])
        n = len(want["rep"])
        assert d._raw("result", 0, n + 1, None, None, None) == INVALID and d._raw("result", -1, 1, None, None, None) == INVALID
        assert d._raw("umis", n, 1, None, None) == INVALID and d._raw("result", n, 0, None, None, None) == 0
        d.close()


def test_separator_and_tag_parameters():
    run = [dc.name_row(b"a:AAC_x", [(0, 5, dc.cig("30M"), 0)], b"BCZ" + b"GGT\0"), dc.name_row(b"b:AAC", [(0, 5, dc.cig("30M"), 0)], b"BCZ" + b"GGT\0"),
           dc.name_row(b"c:AAG", [(0, 5, dc.cig("30M"), 0)], b"BCZ" + b"GGA\0")]
    groups = dc.records_of(run)
    stream, tb = dc.stream_of(groups), dc.tables_of(run)
    for source, params, kw in (("name", {"umi_sep": ":"}, {"sep": b":"}), ("tag", {"umi_tag": "BC"}, {"tag": b"BC"})):
        umis, _ = dc.umis_of(groups, source, **kw)
        rep = dc.molecules_of("unique", dc.signatures_of(groups), umis)
        d = lib.Dedup(method=0, umi_source=dc.SOURCES[source], **params)
        _fill(d, tb, stream, "host")
        d.finish()
        assert np.array_equal(d.umis(0, 3)[0], dc.umi_matrix(umis)[0]) and np.array_equal(d.result()[0], rep), source
        d.close()


@pytest.mark.parametrize("bits", [1, 4, 64])
def test_hash_width_changes_nothing(bits):
    run, groups, stream, tb = _input("standard")
    want = _expected("standard", False, "directional", "name")
    d = lib.Dedup()
    _fill(d, tb, stream, "dev3")
    d.set_param("hash_bits", bits)   # (before finish is early enough)
    st = _assert_result(d, want, bits)
    assert (st["collisions"] > 0) == (bits < 64), st
    d.close()


# ---- shapes ----------------------------------------------------------------------------------------------------------------------
def test_the_chain_needs_every_sweep_and_is_one_molecule():
    run, groups, stream, tb = _input("chain")
    want = _expected("chain", False, "directional", "name")
    assert want["counts"] == (96, 1, 95)
    d = lib.Dedup()
    _fill(d, tb, stream, "host")
    st = _assert_result(d, want, "chain")
    assert st["max_group_nodes"] == 96 and 95 <= st["sweeps"] <= st["max_group_nodes"] and st["edges"] == 2 * 95
    d.close()


def test_the_paper_network():
    run, groups, stream, tb = _input("paper")
    for method, mols in (("directional", 2), ("unique", 6)):
        want = _expected("paper", False, method, "name")
        assert want["counts"][1] == mols
        d = lib.Dedup(method=dc.METHODS[method])
        _fill(d, tb, stream, "dev1")
        _assert_result(d, want, method)
        d.close()


@pytest.mark.parametrize("kind", ["no-dups", "one"])
def test_small_inputs(kind):
    run, groups, stream, tb = _input(kind)
    want = _expected(kind, False, "directional", "name")
    assert want["counts"][2] == 0
    for how in ("host", "dev1"):
        d = lib.Dedup(keep_records=1)
        _fill(d, tb, stream, how)
        _assert_result(d, want, (kind, how))
        got, _ = _drain(d, BIG)
        assert np.array_equal(got, stream)
        d.close()


def test_no_names_at_all():
    d = lib.Dedup(keep_records=1)
    assert d.finish() == (0, 0, 0)
    assert d.result()[0].size == 0 and not d.hist().any() and d.next_records(BIG).n_rows == 0
    assert d.flags()[1] == 0
    d.close()
    d = lib.Dedup()   # names, none of them with rows
    tb = dc.tables_of([dc.name_row(b"x_AC", []), dc.name_row(b"y_AC", [])])
    _fill(d, tb, np.zeros(0, np.uint8), "host")
    assert d.finish() == (2, 0, 0)
    rep, gf, dup = d.result()
    assert list(rep) == [dc.NONE] * 2 and list(gf) == [dc.NONE] * 2 and not dup.any()
    d.close()


# ---- records ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mark", [0, 1])
def test_records_equal_the_expected_stream(mark):
    run, groups, stream, tb = _input("standard")
    want = _expected("standard", False, "directional", "name")
    exp = dc.expected_stream(groups, want["dup"], mark)
    assert (exp.size == stream.size) == bool(mark) and exp.size > 0
    n_spilled = sum(1 for g in groups for r in g if b"CGBI" in r)
    assert n_spilled > 10   # records in the CG:B,I form pass through as they are
    for mb, how in ((BIG, "dev1"), (4096, "host3"), (1, "dev3")):   # (three adds: the arena grows twice)
        d = lib.Dedup(keep_records=1, mark=mark)
        _fill(d, tb, stream, how)
        _assert_result(d, want, (mark, mb))
        got, pieces = _drain(d, mb)
        assert got.size == exp.size and np.array_equal(got, exp), (mark, mb)
        assert all(b <= mb or r == 1 for b, r in pieces) and (mb != 1 or len(pieces) == d.stats()["records_out"])
        assert d.stats()["held_bytes"] > stream.size
        d.close()


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_calls_in_the_wrong_order_and_bad_tables():
    run, groups, stream, tb = _input("no-dups")
    want = _expected("no-dups", False, "directional", "name")
    d = lib.Dedup()
    assert d._raw("result", 0, 0, None, None, None) == INVALID and d._raw("hist", None) == INVALID   # before finish
    assert d._raw("set_param", b"method", 2) == INVALID and d._raw("set_param", b"hist_max", 0) == INVALID and d._raw("set_param", b"nothing", 1) == INVALID
    rec_off = lib.Sorter.row_offsets(stream)
    recs = lib.BrDeviceBam(stream.ctypes.data, stream.size, rec_off.ctypes.data, len(rec_off) - 1)
    a, cg, pl, ro, go = tb["a"], tb["cigar"], tb["pool"], tb["row_off"], tb["group_off"]

    def add(recs=recs, a=a, cg=cg, pl=pl, ro=ro, go=go, n_rows=len(a)):
        return d.add_raw(recs, a.ctypes.data, cg.ctypes.data, pl.ctypes.data, ro.ctypes.data, n_rows, len(pl), go.ctypes.data, len(go) - 1, False)
    assert add(recs=None) == INVALID   # the records are required
    bad_go = go.copy(); bad_go[3] = bad_go[5]
    assert add(go=bad_go) == INVALID   # names that descend
    bad_ro = ro.copy(); bad_ro[4] = bad_ro[2]
    assert add(ro=bad_ro) == INVALID
    assert add(n_rows=len(a) - 1) == INVALID   # recs->n_rows != rows->n_rows
    bad_off = rec_off.copy(); bad_off[7] = bad_off[5]
    assert d.add_raw(lib.BrDeviceBam(stream.ctypes.data, stream.size, bad_off.ctypes.data, len(bad_off) - 1), a.ctypes.data, cg.ctypes.data, pl.ctypes.data,
                     ro.ctypes.data, len(a), len(pl), go.ctypes.data, len(go) - 1, False) == INVALID
    big_a, big_cg = a.copy(), cg.copy()
    big_a[9, 2] = (int(big_a[9, 2]) & 0xff000000) | 3; big_cg[9] = len(pl) - 1   # a pooled CIGAR that leaves the pool
    assert add(a=big_a, cg=big_cg) == INVALID
    assert d.stats()["names"] == 0 and d.umis(0, 0)[0].shape == (0, 32)   # nothing was added
    assert add() == 0
    assert d._raw("set_param", b"method", 0) == INVALID   # after the first add
    _assert_result(d, want, "after the refusals")
    assert add() == INVALID and d._raw("finish", None, None, None) == INVALID   # after finish
    assert d._raw("next", BIG, lib.C.byref(lib.BrDeviceBam())) == INVALID   # without "keep_records"
    d.close()


def test_the_arena_cap():
    run, groups, stream, tb = _input("no-dups")
    want = _expected("no-dups", False, "directional", "name")
    d = lib.Dedup(keep_records=1, max_bytes=stream.size - 1)
    with pytest.raises(lib.BrambleError):
        _fill(d, tb, stream, "host")
    assert d.stats()["names"] == 0
    d.close()
    d = lib.Dedup(keep_records=1, max_bytes=stream.size)
    _fill(d, tb, stream, "host3")
    _assert_result(d, want, "cap")
    assert np.array_equal(_drain(d, BIG)[0], stream)
    d.close()


# ---- the quant hook --------------------------------------------------------------------------------------------------------------
def _quant(n_tx, boot=4):
    q = lib.Quant(n_tx)
    q.set_param("keep_names", 1)
    q.set_param("bootstraps", boot)
    q.set_param("boot_seed", 11)
    return q


def _quant_everything(q):
    out = {"finish": q.finish()[1], "classes": q.classes()}
    q.em()
    out["result"] = q.result()
    out["name_cls"] = q.name_classes()
    q.bootstrap()
    out["boot"] = q.boot_theta()
    out["unassigned"] = q.stats()["n_unassigned"]
    return out


def _same(x, y):
    if isinstance(x, dict):
        return set(x) == set(y) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, (tuple, list)):
        return len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    if isinstance(x, np.ndarray):
        return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8))
    return x == y


@pytest.mark.parametrize("where", ["host", "device", "object"])
def test_drop_names_equals_a_quantifier_that_never_saw_them(where):
    import torch
    run, groups, stream, tb = _input("standard")
    want = _expected("standard", False, "directional", "name")
    d = lib.Dedup()
    _fill(d, tb, stream, "dev1")
    d.finish()
    dup = d.result()[2]
    assert np.array_equal(dup, want["dup"]) and dup.sum() > 300
    multi = [i for i in np.flatnonzero(dup) if len({r[0] for r in run[i]["rows"]}) > 1]
    assert multi   # a multi-transcript name among the duplicates
    n_tx = int(tb["a"][:, 0].max()) + 1
    # the yardstick: the same names, the dropped ones' row ranges emptied
    emptied = [dc.name_row(nm["name"], [] if dup[i] else nm["rows"]) for i, nm in enumerate(run)]
    tb2 = dc.tables_of(emptied)
    q2 = _quant(n_tx)
    q2.add_host(tb2["a"], tb2["row_off"], tb2["group_off"])
    exp = _quant_everything(q2)
    q = _quant(n_tx)
    q.add_host(tb["a"], tb["row_off"], tb["group_off"])
    assert q._raw("drop_names", dup.ctypes.data, len(dup) - 1, 0, None) == INVALID   # a wrong n: refused, nothing changes
    flags = {"host": dup, "device": torch.from_numpy(dup).cuda(), "object": d}[where]
    assert q.drop_names(flags) == int(dup.sum())
    got = _quant_everything(q)
    for k in exp:
        assert _same(got[k], exp[k]), k
    assert got["unassigned"] >= int(dup.sum()) and np.all(got["name_cls"][dup != 0] == dc.NONE)
    # and without the call the quantifier counts the copies
    q3 = _quant(n_tx)
    q3.add_host(tb["a"], tb["row_off"], tb["group_off"])
    assert not _same(_quant_everything(q3)["classes"], exp["classes"])
    for o in (q, q2, q3, d):
        o.close()


# ---- the context's last call -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_add_last_on_projected_records(mode):
    """the rows, names and records a projection call leaves in HBM, both methods, against the restatement on the call's own records;
    then the same names in three calls' worth of adds and the results are the same"""
    import torch
    from tests.test_gpu_collate import _cat
    annd, recs = _cli_input(mode)
    stream = _cat(recs)
    off, ln, _, _ = lib.bam_split(stream)
    ctx = lib.Context(lib.Index(annd, device=0))
    r = lib.BrDeviceRecords()
    held = (torch.from_numpy(stream.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(), torch.from_numpy(ln.astype(np.int32)).cuda())
    r.blob, r.rec_off, r.n_aln, r.rec_len = held[0].data_ptr(), held[1].data_ptr(), len(ln), held[2].data_ptr()
    db, cnt = ctx.project_bam_resident_kept(lib.make_config(lr=int(mode == "ont")), r, np.arange(len(annd["refnames"]), dtype=np.int32))
    objs = {m: lib.Dedup(method=dc.METHODS[m], keep_records=1, mark=1) for m in ("directional", "unique")}
    for d in objs.values():
        d.add_last(ctx)
    out = ctx.device_bam_download(db)
    groups = [g for _, g in dc.name_groups(out)]
    assert cnt["n_rows"] == sum(len(g) for g in groups) > 1000
    umis, ucnt = dc.umis_of(groups)
    sigs = dc.signatures_of(groups)
    for m, d in objs.items():
        want = dc.molecules_of(m, sigs, umis)
        n, mols, dups = d.finish()
        assert (mols, dups) == dc.counts_of(want)[1:] and dups > 0.3 * len(groups), m
        rep, gf, dup = d.result()
        named = np.flatnonzero(rep != dc.NONE)   # the names with records, in the order of the output's groups
        assert len(named) == len(groups) and n >= len(groups)
        assert np.array_equal(np.searchsorted(named, rep[named]), want) and np.array_equal(np.searchsorted(named, gf[named]), dc.groups_of(sigs)), m
        assert np.array_equal(dup[named], dc.dup_of(want)) and not dup[rep == dc.NONE].any()
        assert np.array_equal(d.umis(0, n)[0][named], dc.umi_matrix(umis)[0]) and d.stats()["no_umi"] == ucnt["no_umi"]
        got, _ = _drain(d, 1 << 16)
        assert np.array_equal(got, dc.expected_stream(groups, dc.dup_of(want), True)), m
        d.close()


def test_add_last_refuses_a_flat_batch_call():
    """a flat batch call leaves rows and no records"""
    from tests.test_gpu_coverage_weight import _fill_last, _tables
    flat = lib.Dedup()
    with pytest.raises(lib.BrambleError):
        _fill_last([flat], _tables("pe")["tb"])
    assert flat.stats()["names"] == 0 and flat.finish() == (0, 0, 0)
    flat.close()


# ---- the command line ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cli_input(mode):
    """(annotation dict, the framed records of a synthetic input, paired or long reads, through with_umis)"""
    from tests.test_gpu_collate import _inputs
    annd, recs, _ = _inputs(mode)
    return annd, tuple(dc.with_umis_records(recs[:1500]))


LINE = re.compile(r"\[bramble\] dedup: (\d+) molecules of (\d+) read names \((\d+) duplicates, (\d+) without UMI; (\d+) position groups; "
                  r"method (unique|directional); add \d+\.\d\ds, finish \d+\.\d\ds\)$")


@pytest.mark.parametrize("fmt", ["bam", "sam", "collate", "ont"])
def test_cli_dedup(tmp_path, fmt):
    import random
    from bramble_amd import synth
    from tests import bamio
    from tests.test_collate_cpu import read_name
    from tests.test_gpu_collate import _cat, _files, _report, _run, _strip
    annd, recs = _cli_input("ont" if fmt == "ont" else "pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)

    def infile(records, tag):
        bam, hdr = _files(tmp_path, annd, _cat(records), tag)
        if fmt != "sam":
            return bam
        sam = str(tmp_path / (tag + ".sam"))
        open(sam, "wb").write(hdr.encode() + synth.records_to_sam(_cat(records), annd["refnames"]))
        return sam
    extra = ["-G", gtf] + (["--collate"] if fmt == "collate" else []) + (["--lr"] if fmt == "ont" else [])
    given = list(recs)
    if fmt == "collate":
        random.Random(3).shuffle(given)
    src = infile(given, "in")
    plain = _run([src] + extra + ["--quant", str(tmp_path / "q0.tsv")], str(tmp_path / "o0.bam"))
    t0, refs0, s0 = bamio.read_bam(str(tmp_path / "o0.bam"))
    groups = dc.name_groups(s0)
    assert len(set(nm for nm, _ in groups)) == len(groups) > 300
    only = [g for _, g in groups]
    umis, cnt = dc.umis_of(only)
    sigs = dc.signatures_of(only)
    rep = dc.molecules_of("directional", sigs, umis)
    dup = dc.dup_of(rep)
    assert dup.sum() > 0.3 * len(dup) and not np.array_equal(rep, dc.molecules_of("unique", sigs, umis))
    is_dup = {nm for (nm, _), d in zip(groups, dup) if d}
    # the input from which the duplicate names were removed beforehand, quantified without --dedup
    ordered = list(recs) if fmt != "collate" else [r for _, g in sorted(_first_seen(given).items(), key=lambda kv: kv[1][0]) for r in g[1]]
    kept = [r for r in ordered if bytes(read_name(r)[:-1]) not in is_dup]
    _run([infile(kept, "kept")] + ["-G", gtf] + (["--lr"] if fmt == "ont" else []) + ["--quant", str(tmp_path / "q2.tsv")], str(tmp_path / "o2.bam"))
    for mode in ("remove", "mark"):
        d = tmp_path / mode
        d.mkdir()
        r = _run([src] + extra + ["--quant", str(d / "q.tsv"), "--dedup", "directional", "--dedup-stats", str(d / "s.tsv"), "--dedup-bam", str(d / "d.bam"),
                                  "--dedup-bam-mode", mode], str(d / "o.bam"))
        t1, refs1, s1 = bamio.read_bam(str(d / "o.bam"))
        assert _strip(t1) == _strip(t0) and refs1 == refs0 and np.array_equal(s1, s0)   # the main output
        assert _report(r) == _report(plain)                                              # and the final report
        line = [l for l in r.stdout.decode().split("\n") if l.startswith("[bramble] dedup:")]
        assert len(line) == 1 and LINE.match(line[0]), line
        m = LINE.match(line[0])
        n, mols, dups = dc.counts_of(rep)
        assert (int(m.group(1)), int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(6)) == (mols, dups, cnt["no_umi"], len(set(sigs)), "directional")
        assert len(groups) <= int(m.group(2)) <= len(set(bytes(read_name(x)) for x in recs))
        t2, refs2, s2 = bamio.read_bam(str(d / "d.bam"))
        assert _strip(t2) == _strip(t0) and refs2 == refs0
        exp = dc.expected_stream(only, dup, mode == "mark")
        assert s2.size == exp.size and np.array_equal(s2, exp), mode
        hist = dc.hist_of(rep)
        assert open(str(d / "s.tsv")).read() == "".join("%d\t%d\n" % (k, v) for k, v in enumerate(hist) if v)
        assert open(str(d / "q.tsv")).read() == open(str(tmp_path / "q2.tsv")).read()
        assert open(str(d / "q.tsv")).read() != open(str(tmp_path / "q0.tsv")).read()


def _first_seen(records):
    """read name -> (index of its first record, its records in input order): the order --collate gives the groups"""
    from tests.test_collate_cpu import read_name
    out = {}
    for i, r in enumerate(records):
        out.setdefault(bytes(read_name(r)), (i, []))[1].append(r)
    return out


@pytest.mark.parametrize("extra,word", [
    (["--quant", "q.tsv", "--quant-bam", "p.bam", "--dedup", "directional"], b"--dedup not with --quant-bam"),
    (["--quant", "q.tsv", "--coverage", "c.bg", "--coverage-weight", "em", "--dedup", "unique"], b"--dedup not with --coverage-weight em"),
    (["--dedup-stats", "s.tsv"], b"need --dedup"),
    (["--dedup", "unique", "--dedup-bam-mode", "mark"], b"--dedup-bam-mode needs --dedup-bam"),
])
def test_cli_refusals(tmp_path, extra, word):
    import subprocess
    from tests.test_gpu_collate import BIN
    r = subprocess.run([BIN, "in.bam", "-G", "g.gtf", "-o", "o.bam"] + extra, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr[:300]
    assert os.listdir(str(tmp_path)) == []

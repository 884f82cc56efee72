"""The command line's --quant, --quant-eff-length and --coverage on the routes a production run takes.  The default bundle is
1 000 000 records, so a real short-read run feeds the accumulators from direct rows; the other command-line tests have inputs of a
few thousand reads and never leave the small-batch path.  Here 40 000 pairs -- one default bundle of more than 65 536 alignments,
the smallest shape at which the program itself leaves that path -- go through bramble three times: the default bundle (direct
rows), --bundle-size 5000 (the small-batch path) and BRAMBLE_AMD_DIRECT_ROWS=0 (the match table).  The output and the six side
files are the same bytes each time, the records are the oracle's, and the side files are what the yardsticks say on the oracle's
rows.

The long-read sequence of a production run (ordinary match table, then predicted launches) is held to the yardsticks at API level,
tests/test_gpu_consumers_routes.py::test_a_run_of_long_read_calls: at the command line it needs two bundles of more than 65 536
long reads, and generating, projecting on the oracle and measuring with the Python yardsticks ONE bundle of 70 000 of the
generator's ont reads (320 550 rows, 6.0 M CIGAR words) takes 13 s before the program has run once -- a test here has about ten.

The consumers that take a bundle's records beside its rows -- --dedup, --cells, --quant-bam -- go the same way in the second test,
on the same pairs with UMIs and cell barcodes in their names."""
import functools
import os
import subprocess

import numpy as np
import pytest

from bramble_amd import lib, synth
from oracle import oracle_binding as ob
from tests import bamio
from tests import route_cases as rc
from tests.test_gpu_collate import BIN, _files
from tests.test_gpu_coverage import _assert_summary, _bedgraph
from tests.test_gpu_quant import _body
from tests.test_gpu_quant_fld import _fld_tsv, _parse_eff_tsv
from tests.test_quant_cpu import parse_eq_classes, unique_ambig
from tests.test_quant_fld_cpu import packed_of

pytestmark = pytest.mark.gpu

SIDE = ("q.tsv", "eq.txt", "fld.tsv", "bedgraph", "cov.tsv")


@functools.lru_cache(maxsize=None)
def paired_expectations():
    """the input with its transcripts numbered as the command line's guide loader numbers them, the oracle's stream and rows of
    it, and the yardsticks over those rows"""
    ann, b = rc.cli_pairs()
    annd = ann.as_dict()
    annd = dict(annd, transcripts=[annd["transcripts"][t] for t in bamio.guide_order(annd)])
    stream, roff, rlen = synth.Annotation.frame_records(b)
    assert len(roff) == b["n_aln"] > rc.SMALL_N
    oi = ob.OracleIndex(annd)
    orc, _, _, _ = ob.run_bam(oi, ob.make_flags(), stream, roff, rlen, np.arange(len(annd["refnames"]), dtype=np.int32))
    lens = rc.oracle_lens(oi)
    tables = rc.yardstick_rows(orc, rc.group_starts(b))
    return {"annd": annd, "batch": b, "stream": stream, "orc_stream": orc["bam_stream"], "lens": lens, "tables": tables,
            "want": rc.yardsticks(*tables, lens)}


def _bramble(args, env=None):
    r = subprocess.run([BIN] + args, capture_output=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr.decode() + r.stdout.decode()
    return r


def test_cli_paired_run_on_its_production_route(tmp_path):
    e = paired_expectations()
    annd, lens, want = e["annd"], e["lens"], e["want"]
    rows, row_off, group_off = e["tables"]
    n_tx = len(lens)
    # a default context sends these records down direct rows
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, "small")
    route, _ = rc.run_route(ctx, "small", lib.make_config(), e["batch"])
    assert route == "direct"
    ctx.close()
    # the library's own EM on the oracle's rows: the floats are compared as printed
    q = rc.new_quant(n_tx, lens)
    q.add_rows_host(*packed_of(rows), row_off, group_off)
    q.finish()
    q.em()
    api = q.result()
    q.close()
    idx.close()

    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, e["stream"], "in")

    def paths(tag):
        return [str(tmp_path / ("%s.%s" % (tag, ext))) for ext in ("out.bam",) + SIDE]
    runs = (("default", [], None), ("small", ["--bundle-size", "5000"], None), ("match_table", [], {"BRAMBLE_AMD_DIRECT_ROWS": "0"}))
    for tag, more, env in runs:
        o, qt, eq, fld, bed, cov = paths(tag)
        _bramble([in_bam, "-G", gtf, "-o", o, "--quant", qt, "--quant-classes", eq, "--quant-eff-length", "--quant-fld", fld,
                  "--coverage", bed, "--coverage-summary", cov] + more, env)
    # the three runs: the same records (the header but for the @PG line that names the command line) and the same side files
    o, qt, eq, fld, bed, cov = paths("default")
    head, recs = _body(o, False)
    for tag in ("small", "match_table"):
        other = paths(tag)
        h1, s1 = _body(other[0], False)
        assert h1 == head and np.array_equal(s1, recs), tag
        for mine, theirs in zip(paths("default")[1:], other[1:]):
            assert open(mine, "rb").read() == open(theirs, "rb").read(), (tag, os.path.basename(mine))
    # the records are the oracle's
    assert np.array_equal(recs, e["orc_stream"]) and len(recs) > 10 ** 7
    # the classes
    tx_names = [t["id"] for t in annd["transcripts"]]
    cl = want["classes"]
    names, labels, counts = parse_eq_classes(open(eq).read())
    assert names == tx_names and labels == cl["labels"] and counts == cl["counts"]
    # the table: integer columns exactly, the effective length as the yardstick prints it, the floats as the API's print
    got = _parse_eff_tsv(open(qt).read())
    uniq, ambig = unique_ambig(cl, n_tx)
    assert [f[0] for f in got] == tx_names and [int(f[1]) for f in got] == lens.tolist()
    assert [int(f[5]) for f in got] == uniq.tolist() and [int(f[6]) for f in got] == ambig.tolist()
    assert [f[2] for f in got] == ["%.3f" % v for v in want["eff"]]
    assert [f[3] for f in got] == ["%.6f" % v for v in api["theta"]] and [f[4] for f in got] == ["%.6f" % v for v in api["tpm"]]
    # the fragment histogram and the coverage
    assert want["fld"]["n_obs"] > 1000 and open(fld).read() == _fld_tsv(want["fld"]["hist"])
    assert len(want["cov"][0]["runs"][0]) > 50000 and open(bed).read() == _bedgraph(want["cov"][0], tx_names)
    _assert_summary(open(cov).read(), want["cov"][0], tx_names, lens, "default")


# ---- --dedup, --cells and --quant-bam: the consumers that take a bundle's records beside its rows ------------------------------------
@functools.lru_cache(maxsize=None)
def decorated_expectations():
    """the same 40 000 pairs with UMIs and cell barcodes in their names (record_route_cases.decorate_lightly), the oracle's stream
    of them, and what --dedup directional beside --cells says of that stream: the whitelist's resolution of the barcodes, the
    molecules per cell, and the matrix of the names that are no duplicates over the transcripts"""
    from tests import cells_cases as cc
    from tests import dedup_cases as dc
    from tests import record_route_cases as rr
    from tests import whitelist_cases as wc
    ann, b = rc.cli_pairs()
    annd = ann.as_dict()
    annd = dict(annd, transcripts=[annd["transcripts"][t] for t in bamio.guide_order(annd)])
    recs = rr.decorate_lightly(rr.records_of_batch(b))
    assert len(recs) > rc.SMALL_N
    stream, roff, rlen = rr.split3(recs)
    oi = ob.OracleIndex(annd)
    orc, _, _, _ = ob.run_bam(oi, ob.make_flags(), stream, roff, rlen, np.arange(len(annd["refnames"]), dtype=np.int32))
    groups = [g for _, g in dc.name_groups(orc["bam_stream"])]
    whitelist = wc.cli_whitelist()[1]
    umis, ucnt = dc.umis_of(groups)
    _, status, resolved = wc.resolve(whitelist, wc.observed_of(groups), wc.CORRECT["1mm"])
    rep, gf = cc.per_cell_molecules("directional", groups, umis, resolved)
    dup = dc.dup_of(rep)
    name_cls, classes = cc.classes_of(groups, dup)
    model = cc.model_of(resolved, name_cls, classes, np.arange(oi.num_transcripts(), dtype=np.uint32))
    return {"annd": annd, "recs": recs, "stream": stream, "orc_stream": orc["bam_stream"], "groups": groups, "whitelist": whitelist, "rep": rep, "dup": dup,
            "no_umi": ucnt["no_umi"], "position_groups": len(set(gf.tolist()) - {dc.NONE}), "model": model, "matrix": cc.matrix_of(model, "uniform"),
            "plain_molecules": dc.counts_of(dc.molecules_of("directional", dc.signatures_of(groups), umis))[1]}


def _bam_body(path):
    from tests.test_gpu_collate import _strip
    text, refs, s = bamio.read_bam(path)
    return _strip(text), refs, bytes(s)


def test_cli_record_consumers_on_their_production_route(tmp_path):
    """--dedup with its stats file and --dedup-bam, --cells with a whitelist, and --quant-bam, on the default bundle (direct rows)
    and with --bundle-size 5000 (the small-batch path).  --dedup is refused beside --quant-bam (the duplicate names have no
    class), so each way is two runs: one with --dedup and --cells, one with --quant-bam.  The main output and every side file are
    the same bytes on both ways (the @PG line names the command line, the dedup line's times are not compared); the default
    run's records are the oracle's, and its dedup counts, stats file, marked records and cells matrix are what the restatements
    say on the oracle's stream.

    Measured on the MI355X, test_cli_paired_run_on_its_production_route taking 7.3 to 7.7 s (the parent commit's code; 5.6 s
    behind other tests in one process): with a third way (BRAMBLE_AMD_DIRECT_ROWS=0, the match table) and --cells-filter
    topcells this test took 12.3 s; the match-table way was dropped first, then the calling method, and it takes 9.3 to 9.7 s:
    4.6 s for the input, the oracle and the Python restatements over 466 026 projected records (they read every record whatever
    the number of copied names), 1.7 s for the four runs, the rest for writing the input and reading 120 MB of BAM back.  The
    match table under these consumers is held to the same restatements at API level,
    tests/test_gpu_record_consumers_routes.py; the calling method beside --cells by tests/test_gpu_cli_cellcall.py."""
    from tests import dedup_cases as dc
    from tests.test_gpu_cells import _parse_cells
    from tests.test_gpu_dedup import LINE
    from tests import record_route_cases as rr
    e = decorated_expectations()
    annd = e["annd"]
    # a default context sends these records down direct rows
    idx = lib.Index(annd, device=0)
    ctx = rc.new_context(idx, "small")
    route, got, _ = rr.run_route(ctx, "small", lib.make_config(), e["recs"], np.arange(len(annd["refnames"]), dtype=np.int32))
    assert route == "direct" and np.array_equal(got, e["orc_stream"])
    ctx.close()
    idx.close()
    gtf, wl = str(tmp_path / "g.gtf"), str(tmp_path / "wl.txt")
    bamio.write_gtf(gtf, annd)
    open(wl, "wb").write(b"".join(b + b"\n" for b in e["whitelist"]))
    in_bam, _ = _files(tmp_path, annd, e["stream"], "in")
    ways = (("default", [], None), ("small", ["--bundle-size", "5000"], None))
    cells_files = ("matrix.mtx", "barcodes.tsv", "features.tsv", "cells.tsv")
    out, lines = {}, {}
    for tag, more, env in ways:
        d = tmp_path / tag
        d.mkdir()
        p = lambda name: str(d / name)   # noqa: E731
        r = _bramble([in_bam, "-G", gtf, "-o", p("a.bam"), "--quant", p("qa.tsv"), "--dedup", "directional", "--dedup-stats", p("s.tsv"),
                      "--dedup-bam", p("d.bam"), "--dedup-bam-mode", "mark", "--cells", p("c."), "--cells-features", "transcript",
                      "--cells-multi", "uniform", "--cells-whitelist", wl] + more, env)
        _bramble([in_bam, "-G", gtf, "-o", p("b.bam"), "--quant", p("qb.tsv"), "--quant-bam", p("p.bam")] + more, env)
        assert sorted(os.listdir(str(d))) == sorted(["a.bam", "b.bam", "d.bam", "p.bam", "qa.tsv", "qb.tsv", "s.tsv"] + ["c." + n for n in cells_files])
        out[tag] = {n: _bam_body(p(n)) for n in ("a.bam", "b.bam", "d.bam", "p.bam")}
        out[tag].update({n: open(p(n), "rb").read() for n in ["qa.tsv", "qb.tsv", "s.tsv"] + ["c." + n for n in cells_files]})
        line = [l for l in r.stdout.decode().split("\n") if l.startswith("[bramble] dedup:")]
        assert len(line) == 1 and LINE.match(line[0]), line
        lines[tag] = LINE.match(line[0]).groups()       # (the times behind the counts are not among the groups)
    for name in out["default"]:
        assert out["small"][name] == out["default"][name], name
    assert lines["small"] == lines["default"]
    # the default run against the oracle and the restatements
    mine = out["default"]
    assert mine["a.bam"][2] == mine["b.bam"][2] == bytes(e["orc_stream"]) and len(e["orc_stream"]) > 10 ** 7
    n, mols, dups = dc.counts_of(e["rep"])
    m = lines["default"]
    assert (int(m[0]), int(m[2]), int(m[3]), int(m[4]), m[5]) == (mols, dups, e["no_umi"], e["position_groups"], "directional")
    assert dups > 1000 and mols > e["plain_molecules"]     # (the same UMI and placements in two cells are two molecules)
    assert mine["s.tsv"].decode() == "".join("%d\t%d\n" % (k, v) for k, v in enumerate(dc.hist_of(e["rep"])) if v)
    assert mine["d.bam"][2] == bytes(dc.expected_stream(e["groups"], e["dup"], True))
    assert len(mine["p.bam"][2]) == len(e["orc_stream"]) + 7 * sum(len(g) for g in e["groups"])   # ZW:f behind every record
    model, want = e["model"], e["matrix"]
    kind, dims, rows, barcodes, features, table = _parse_cells(str(tmp_path / "default" / "c."))
    assert kind == "real" and dims == (len(annd["transcripts"]), len(model["cells"]), len(want["feature"])) and len(model["cells"]) == 12
    assert barcodes == [b.decode() for b in model["cells"]]
    cell_of = np.repeat(np.arange(len(model["cells"])), np.diff(want["off"].astype(np.int64)))
    assert [(f, c) for f, c, _, _ in rows] == [(int(f) + 1, int(c) + 1) for f, c in zip(want["feature"], cell_of)]
    assert [text for _, _, _, text in rows] == ["%.10g" % v for v in want["value"]]     # one iteration: the values as printed
    assert [t[:6] for t in table[1:]] == [[b.decode()] + [str(int(want[k][i])) for k in ("names", "unique", "multi", "features", "iterations")]
                                          for i, b in enumerate(model["cells"])]
    assert int(want["multi"].sum()) > 1000

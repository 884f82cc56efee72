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
generator's ont reads (320 550 rows, 6.0 M CIGAR words) takes 13 s before the program has run once -- a test here has about ten."""
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

"""--cells-filter on the command line: the three new files against lib.CellCall run on the matrix the same run wrote, the report
line, and every other output as it is without the switch."""
import os
import re
import subprocess

import numpy as np
import pytest

from bramble_amd import lib

pytestmark = pytest.mark.gpu

LINE = re.compile(r"^\[bramble\] cell calling: (\d+) of (\d+) cells called \((\d+) simple, (\d+) by emptydrops of (\d+) candidates; threshold (\d+); "
                  r"ambient (\d+) counts over (\d+) barcodes, (\d+) features; (\d+) sims; method (topcells|cr2\.2|emptydrops); "
                  r"rank \d+\.\d\ds, simulate \d+\.\d\ds\)$")
OLD = ("matrix.mtx", "barcodes.tsv", "features.tsv", "cells.tsv")
NEW = ("filtered_matrix.mtx", "filtered_barcodes.tsv", "calls.tsv")
SWITCHES = {"topcells": (["--cells-expected", "4"], dict(method=0, expected=4)),
            "cr2.2": (["--cells-expected", "4", "--cells-filter-ratio", "2", "--cells-filter-percentile", "0.9"],
                      dict(method=1, expected=4, ratio=2.0, percentile=0.9)),
            "emptydrops": (["--cells-expected", "2", "--cells-filter-ratio", "1.5", "--cells-ed-window", "8,12", "--cells-ed-umi-min", "1",
                            "--cells-ed-umi-frac", "0", "--cells-ed-sims", "200", "--cells-ed-fdr", "0.5", "--cells-ed-candidates", "3",
                            "--quant-seed", "7"],
                           dict(method=2, expected=2, ratio=1.5, ind_min=8, ind_max=12, umi_min=1, umi_frac=0.0, sims=200, fdr=0.5, cand_max=3, seed=7))}


def _matrix(prefix, name="matrix.mtx"):
    """-> (n_features, n_cells, rows of (feature, cell, text)) of a Matrix Market file"""
    body = [l.split() for l in open(prefix + name).read().split("\n")[1:-1] if not l.startswith("%")]
    return int(body[0][0]), int(body[0][1]), [(int(f) - 1, int(c) - 1, v) for f, c, v in body[1:]]


@pytest.mark.parametrize("multi", ["unique", "em"])
@pytest.mark.parametrize("method", sorted(SWITCHES))
def test_cli_cell_filter(tmp_path, method, multi):
    from tests.test_gpu_cells import _cli_files
    from tests import bamio
    from tests.test_gpu_collate import _report, _run, _strip
    bam, gtf, _ = _cli_files(tmp_path)
    base = [bam, "-G", gtf, "--cells-features", "transcript", "--cells-multi", multi]
    p0, p1 = str(tmp_path / "a."), str(tmp_path / "b.")
    plain = _run(base + ["--quant", str(tmp_path / "q0.tsv"), "--cells", p0], str(tmp_path / "o0.bam"))
    switches, params = SWITCHES[method]
    r = _run(base + ["--quant", str(tmp_path / "q1.tsv"), "--cells", p1, "--cells-filter", method] + switches, str(tmp_path / "o1.bam"))
    # everything the run without the switch writes, to the byte
    for name in OLD:
        assert open(p1 + name, "rb").read() == open(p0 + name, "rb").read(), name
    (t0, refs0, s0), (t1, refs1, s1) = bamio.read_bam(str(tmp_path / "o0.bam")), bamio.read_bam(str(tmp_path / "o1.bam"))
    assert _strip(t1) == _strip(t0) and refs1 == refs0 and np.array_equal(s1, s0)   # (the @PG line holds the command line)
    assert open(str(tmp_path / "q1.tsv"), "rb").read() == open(str(tmp_path / "q0.tsv"), "rb").read() and _report(r) == _report(plain)
    assert sorted(x for x in os.listdir(str(tmp_path)) if x.startswith("b.")) == sorted("b." + x for x in OLD + NEW)
    assert not any(x in os.listdir(str(tmp_path)) for x in ("a." + n for n in NEW))
    # the caller on the unique counts of the same cells (--cells-multi unique writes them; the other run's cells are the same)
    unique_prefix = p1
    if multi != "unique":
        unique_prefix = str(tmp_path / "u.")
        _run([bam, "-G", gtf, "--cells-features", "transcript", "--quant", str(tmp_path / "q2.tsv"), "--cells", unique_prefix], str(tmp_path / "o2.bam"))
    F, K, rows = _matrix(unique_prefix)
    assert K == 12 and [c for _, c, _ in rows] == sorted(c for _, c, _ in rows)
    off = np.searchsorted(np.array([c for _, c, _ in rows]), np.arange(K + 1)).astype(np.uint64)
    c = lib.CellCall(**params).run(off, np.array([f for f, _, _ in rows], np.uint32), np.array([int(v) for _, _, v in rows], np.uint32), F)
    status, rank, total = c.calls()
    st, k = c.stats(), c.candidates()
    assert 0 < st["called_simple"] < K and (method != "emptydrops" or (st["fallback"] == 0 and 1 <= st["candidates"] <= 3))
    barcodes = open(p1 + "barcodes.tsv").read().split("\n")[:-1]
    cand_of = {int(cell): j for j, cell in enumerate(k["cell"])}
    want = ["Barcode\tTotal\tRank\tStatus\tLogLik\tLower\tPValue\tPAdj"]
    for i, b in enumerate(barcodes):
        j = cand_of.get(i)
        tail = [".", ".", ".", "."] if j is None else ["%.17g" % k["O"][j], "%d" % k["lower"][j], "%.17g" % k["pval"][j], "%.17g" % k["padj"][j]]
        want.append("\t".join([b, "%d" % total[i], "%d" % rank[i], "%d" % status[i]] + tail))
    assert open(p1 + "calls.tsv").read().split("\n")[:-1] == want
    keep = [i for i in range(K) if status[i]]
    assert open(p1 + "filtered_barcodes.tsv").read().split("\n")[:-1] == [barcodes[i] for i in keep]
    # the filtered matrix: the called cells' rows of the run's own matrix, renumbered
    F1, K1, rows1 = _matrix(p1)
    new = {cell: n for n, cell in enumerate(keep)}
    assert _matrix(p1, "filtered_matrix.mtx") == (F1, len(keep), [(f, new[cell], v) for f, cell, v in rows1 if cell in new])
    assert open(p1 + "filtered_matrix.mtx").readline() == open(p1 + "matrix.mtx").readline()
    line = [l for l in r.stdout.decode().split("\n") if l.startswith("[bramble] cell calling:")]
    assert len(line) == 1 and LINE.match(line[0]), line
    m = LINE.match(line[0])
    assert [int(m.group(i)) for i in range(1, 7)] == [len(keep), K, st["called_simple"], st["called_emptydrops"], st["candidates"], st["threshold"]]
    assert (int(m.group(7)), int(m.group(8)), int(m.group(9))) == (st["ambient_counts"], st["window"], st["active_features"])
    assert int(m.group(10)) == (200 if method == "emptydrops" else 0) and m.group(11) == method
    assert not any(l.startswith("[bramble] cell calling:") for l in plain.stdout.decode().split("\n"))


@pytest.mark.parametrize("extra,word", [
    (["--cells-filter", "cr2.2"], b"--cells-filter needs --cells"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-expected", "5"], b"need --cells-filter"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-ed-sims", "5"], b"need --cells-filter"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "knee"], b"--cells-filter: unknown method"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "topcells", "--cells-expected", "0"], b"--cells-expected: 0 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "topcells", "--cells-expected", "many"], b"--cells-expected: many is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "cr2.2", "--cells-filter-percentile", "1.5"], b"--cells-filter-percentile: 1.5 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "cr2.2", "--cells-filter-ratio", "0.5"], b"--cells-filter-ratio: 0.5 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-window", "9"], b"--cells-ed-window: 9 is not LO,HI"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-window", "9,3"], b"--cells-ed-window: 9,3 is not LO,HI"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-umi-min", "-1"], b"--cells-ed-umi-min: -1 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-umi-frac", "2"], b"--cells-ed-umi-frac: 2 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-candidates", "0"], b"--cells-ed-candidates: 0 is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-fdr", "nan"], b"--cells-ed-fdr: nan is not"),
    (["--quant", "q.tsv", "--cells", "c.", "--cells-filter", "emptydrops", "--cells-ed-sims", "0"], b"--cells-ed-sims: 0 is not"),
])
def test_cli_refuses_bad_values_before_anything_is_projected(tmp_path, extra, word):
    from tests.test_gpu_collate import BIN
    r = subprocess.run([BIN, "in.bam", "-G", "g.gtf", "-o", "o.bam"] + extra, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and word in r.stderr and b"processing alignments" not in r.stdout, r.stderr[:300]
    assert os.listdir(str(tmp_path)) == []

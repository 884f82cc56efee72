"""The command line with every consumer of a run at once -- --sort --write-index, --quant with its switches, --coverage with its
table -- against runs with one feature each (which test_gpu_sort.py, test_gpu_quant.py, test_gpu_quant_fld.py and
test_gpu_coverage.py hold against the oracle), and what a side file that cannot be written leaves behind.

Two runs' BAM files cannot be equal byte for byte from the first byte on: the header's @PG line holds the command line, so the
header's BGZF blocks differ, and with their length every file offset in the BAI.  What is compared instead asks no less: the
header text but for that line, every byte behind the header's blocks (the record section and the EOF block), and the BAI against
the index of its own file's blocks as test_gpu_sort.py::test_cli_write_index builds it -- equal record blocks and a right index of
each file make the two indexes equal but for the shift."""
import gzip
import os
import struct

import pytest

from tests import bamio
from tests.test_gpu_collate import _files, _inputs, _run, _strip
from tests.test_gpu_sort import _voffsets
from tests.test_sort_cpu import bai_bytes

pytestmark = pytest.mark.gpu

SORT = ["--sort", "--write-index"]
SIDE = ("quant.tsv", "classes.txt", "fld.tsv", "cov.bedgraph", "cov.tsv")
REPORT = ("[bramble] sorted ", "[bramble] fragment lengths: ", "[bramble] quantified ", "[bramble] coverage: ")


def _quant(d):
    return ["--quant", d + "/quant.tsv", "--quant-classes", d + "/classes.txt", "--quant-eff-length", "--quant-fld", d + "/fld.tsv"]


def _coverage(d):
    return ["--coverage", d + "/cov.bedgraph", "--coverage-summary", d + "/cov.tsv"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("in")
    annd, _, stream = _inputs("pe")
    gtf = str(d / "g.gtf")
    bamio.write_gtf(gtf, annd)
    return [_files(d, annd, stream, "in")[0], "-G", gtf]


def _record_section(path):
    """(header text, the file's bytes behind the header's blocks, the BAI of those blocks as test_sort_cpu.py builds it)"""
    text, refs, s = bamio.read_bam(path)
    raw = open(path, "rb").read()
    n_header = len(gzip.decompress(raw)) - s.size
    p, u, table = 0, 0, []
    for bs in bamio.bgzf_block_sizes(path):
        table.append((p, u))
        u += struct.unpack_from("<I", raw, p + bs - 4)[0]
        p += bs
    first = next(k for k, (_, uo) in enumerate(table) if uo == n_header)   # the record section starts a block
    recs = bamio.split_stream(s)
    assert len(recs) > 1000
    blocks = [(co, uo - n_header) for co, uo in table[first:-1]]
    return text, raw[table[first][0]:], bai_bytes(recs, _voffsets(recs, blocks, table[-1][0]), len(refs))


def test_every_switch_at_once(tmp_path, inputs):
    dirs = {k: str(tmp_path / k) for k in ("all", "sort", "quant", "coverage")}
    for d in dirs.values():
        os.mkdir(d)
    r = _run(inputs + SORT + _quant(dirs["all"]) + _coverage(dirs["all"]), dirs["all"] + "/out.bam")
    _run(inputs + SORT, dirs["sort"] + "/out.bam")
    _run(inputs + _quant(dirs["quant"]), dirs["quant"] + "/out.bam")
    _run(inputs + _coverage(dirs["coverage"]), dirs["coverage"] + "/out.bam")
    text, body, bai = _record_section(dirs["all"] + "/out.bam")
    text1, body1, bai1 = _record_section(dirs["sort"] + "/out.bam")
    assert _strip(text) == _strip(text1) and body == body1
    assert open(dirs["all"] + "/out.bam.bai", "rb").read() == bai and open(dirs["sort"] + "/out.bam.bai", "rb").read() == bai1
    for name in SIDE:
        single = dirs["quant" if name in SIDE[:3] else "coverage"]
        got = open(os.path.join(dirs["all"], name), "rb").read()
        assert got == open(os.path.join(single, name), "rb").read() and len(got) > 1000, name
    # the four report lines, once each and in this order, directly in front of the final report
    out = r.stdout.decode().split("\n")
    at = out.index("[bramble] final report:")
    assert out[at - 1] == "" and [l[:len(p)] for l, p in zip(out[at - 5:at - 1], REPORT)] == list(REPORT)
    for p in REPORT:
        assert sum(1 for l in out if l.startswith(p)) == 1, p
    assert out[at - 5].endswith(", index written")
    assert sorted(os.listdir(dirs["all"])) == sorted(SIDE + ("out.bam", "out.bam.bai"))


@pytest.mark.parametrize("switch", ["--coverage-summary", "--quant-classes"])   # the last file written; one in the middle
def test_a_side_file_that_cannot_be_written(tmp_path, inputs, switch):
    d = str(tmp_path / "out")
    os.mkdir(d)
    args = inputs + SORT + _quant(d) + _coverage(d)
    args[args.index(switch) + 1] = d + "/no_such_dir/side.txt"
    r = _run(args, d + "/out.bam", ok=False)
    assert r.returncode == 1 and b"no_such_dir/side.txt" in r.stderr
    assert os.listdir(d) == []   # (the inputs lie elsewhere)

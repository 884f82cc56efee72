"""The side files of the command line without a GPU: bramble_amd/csrc/host/cli_output_files.cpp -- SideFile and the five
formatters, which take plain data -- built with tests/cli_output_probe.cpp under the address and undefined-behaviour sanitizers
and run as a child process.  The expected bytes are built here from the probe's inputs (restated below) with the same % formats."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 2 ** 32 + 5
NAMES = ["tA", "tZero", "tB", "tC"]
LENS = [1500, 0, 2 ** 32 + 7, 30]
LISTED = [t for t in range(4) if LENS[t] > 0]   # the transcript without length is in no table
THETA = [5e-7, 123.0, 0.9999995, 1e9 + 0.5]
TPM = [999999.9999995, 7.0, 0.0, 4.4999995e-6]
EFF = [1234.5678, 9.0, 0.0005, 29.9995]
UNIQUE = [0, 9, BIG, 3]
AMBIG = [2 ** 40, 9, 2, BIG]
TEXT, BYTES = b"line one\nline two\n", b"a\0\n\r\r\n\0b"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probe") / "probe")
    subprocess.run(["g++", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                    os.path.join(ROOT, "tests", "cli_output_probe.cpp"), os.path.join(ROOT, "bramble_amd", "csrc", "host", "cli_output_files.cpp")],
                   check=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def formats(probe, tmp_path_factory):
    """(the directory of the formatters' files, the fetch calls of each bedGraph, each bedGraph's return value)"""
    d = str(tmp_path_factory.mktemp("formats"))
    r = subprocess.run([probe, "formats", d], capture_output=True, timeout=60)
    assert r.returncode == 0 and r.stderr == b"", r.stderr.decode()
    fetches, rcs = {}, {}
    for line in r.stdout.decode().splitlines():
        w = line.split()
        if w[0] == "fetch":
            fetches.setdefault(w[1], []).append((int(w[2]), int(w[3])))
        else:
            rcs[w[1]] = int(w[2])
    return d, fetches, rcs


def _read(d, name):
    return open(os.path.join(d, name), "rb").read().decode()


def test_the_rounding_cases_round():
    """the inputs hold what they are meant to hold"""
    assert "%.6f" % THETA[0] in ("0.000000", "0.000001") and "%.6f" % THETA[2] in ("0.999999", "1.000000") and "%.6f" % THETA[3] == "1000000000.500000"
    assert "%.3f" % EFF[0] == "1234.568" and min(UNIQUE[2], AMBIG[0], AMBIG[3]) > 2 ** 32 and len(LISTED) == 3


@pytest.mark.parametrize("eff", [False, True])
def test_quant_table(formats, eff):
    want = "Name\tLength\t%sNumReads\tTPM\tUniqueReads\tAmbigReads\n" % ("EffectiveLength\t" if eff else "")
    for t in LISTED:
        want += "%s\t%d\t" % (NAMES[t], LENS[t]) + ("%.3f\t" % EFF[t] if eff else "") + "%.6f\t%.6f\t%d\t%d\n" % (THETA[t], TPM[t], UNIQUE[t], AMBIG[t])
    assert _read(formats[0], "quant_eff.tsv" if eff else "quant.tsv") == want and want.count("\n") == 4 and "tZero" not in want


def test_quant_classes(formats):
    """the transcripts with a length are numbered 0, 1, 2, and three names are listed; a class on both sides of the one without"""
    classes = [([0, 2], BIG), ([3], 1), ([0, 2, 3], 2 ** 40)]
    sq_of = {t: k for k, t in enumerate(LISTED)}
    want = "3\n3\ntA\ntB\ntC\n" + "".join("%d\t%s\t%d\n" % (len(ts), "\t".join(str(sq_of[t]) for t in ts), n) for ts, n in classes)
    assert _read(formats[0], "classes.txt") == want and want.split("\n")[5] == "2\t0\t1\t%d" % BIG
    assert _read(formats[0], "classes0.txt") == "3\n0\ntA\ntB\ntC\n"


def test_fragment_lengths(formats):
    got = _read(formats[0], "fld.tsv")
    assert got == "FragmentLength\tCount\n" + "".join("%d\t%d\n" % (k, k * k + (2 ** 33 if k == 1000 else 0)) for k in range(1001))
    assert got.count("\n") == 1002


def _run_line(k):
    return "%s\t%d\t%d\t%d\n" % (NAMES[(0, 2, 3)[k % 3]], 10 * k, 10 * k + 5, 2 ** 32 - 1 if k == 5 else k + 1)


@pytest.mark.parametrize("n_runs,pages", [(0, []), (6, [(0, 3), (3, 3)]), (7, [(0, 3), (3, 3), (6, 1)])])
def test_bedgraph_pages(formats, n_runs, pages):
    d, fetches, rcs = formats
    name = "bed%d" % n_runs
    assert fetches.get(name, []) == pages and rcs[name] == 0
    assert _read(d, name) == "".join(_run_line(k) for k in range(n_runs))
    assert n_runs < 6 or "\t4294967295\n" in _read(d, name)


def test_bedgraph_ends_at_the_first_page_that_fails(formats):
    d, fetches, rcs = formats
    assert fetches["bed_fail"] == [(0, 3), (3, 3)] and rcs["bed_fail"] == -3   # (8 runs: the third page is not asked for)
    assert _read(d, "bed_fail") == "".join(_run_line(k) for k in range(3))


def test_coverage_summary(formats):
    records, aligned, covered, deepest = [BIG, 1, 0, 7], [2 ** 40, 1, 1, 10], [1499, 1, BIG, 20], [2 ** 32 - 1, 1, 0, 3]
    want = "Name\tLength\tRecords\tAlignedBases\tCoveredBases\tMaxDepth\tMeanDepth\tBreadth\n"
    for t in LISTED:
        want += "%s\t%d\t%d\t%d\t%d\t%d\t%.6f\t%.6f\n" % (NAMES[t], LENS[t], records[t], aligned[t], covered[t], deepest[t], aligned[t] / LENS[t], covered[t] / LENS[t])
    assert _read(formats[0], "cov.tsv") == want


# ---- SideFile -------------------------------------------------------------------------------------------------------------------
def _sidefile(probe, path, mode="text", fail=0):
    """-> ({"open": 0/1, "tmp": 0/1 while it was open, "close": 0/1, "settle": 0/1}, stderr)"""
    r = subprocess.run([probe, "sidefile", path, mode, str(fail)], capture_output=True, timeout=60)
    assert r.returncode == 0, r.stderr.decode()
    return {k: int(v) for k, v in (l.split() for l in r.stdout.decode().splitlines())}, r.stderr.decode()


def test_sidefile_success(probe, tmp_path):
    p = str(tmp_path / "side.txt")
    got, err = _sidefile(probe, p)
    assert got == {"open": 1, "tmp": 1, "close": 1, "settle": 1} and err == ""
    assert os.listdir(str(tmp_path)) == ["side.txt"] and open(p, "rb").read() == TEXT


def test_sidefile_binary(probe, tmp_path):
    p = str(tmp_path / "side.bin")
    got, err = _sidefile(probe, p, "binary")
    assert got["settle"] == 1 and err == "" and open(p, "rb").read() == BYTES and {0, 10, 13} <= set(BYTES)


def test_sidefile_failed_run(probe, tmp_path):
    p = str(tmp_path / "side.txt")
    open(p, "wb").write(b"from an earlier run\n")
    got, err = _sidefile(probe, p, fail=1)
    assert got == {"open": 1, "tmp": 1, "close": 1, "settle": 1} and err == ""   # (nothing new failed)
    assert os.listdir(str(tmp_path)) == ["side.txt"] and open(p, "rb").read() == b"from an earlier run\n"
    os.remove(p)
    _sidefile(probe, p, fail=1)
    assert os.listdir(str(tmp_path)) == []


def test_sidefile_missing_directory(probe, tmp_path):
    p = str(tmp_path / "no_such_dir" / "side.txt")
    got, err = _sidefile(probe, p)
    assert got == {"open": 0, "tmp": 0, "close": 0, "settle": 1} and err == "error: could not write %s.tmp-bramble\n" % p
    assert os.listdir(str(tmp_path)) == []


def test_sidefile_target_is_a_directory(probe, tmp_path):
    p = str(tmp_path / "taken")
    os.mkdir(p)
    got, err = _sidefile(probe, p)
    assert got == {"open": 1, "tmp": 1, "close": 1, "settle": 0} and err == "error: could not rename %s.tmp-bramble to %s\n" % (p, p)
    assert os.listdir(str(tmp_path)) == ["taken"] and os.listdir(p) == []


def test_sidefile_empty_path(probe, tmp_path):
    r = subprocess.run([probe, "sidefile", "", "text", "0"], capture_output=True, timeout=60, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stderr == b"" and r.stdout.decode().split() == ["open", "0", "tmp", "0", "close", "1", "settle", "1"]
    assert os.listdir(str(tmp_path)) == []

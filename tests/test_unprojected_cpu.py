"""--unprojected without a GPU: the yardstick the GPU tests use (tests/unprojected_cases.py) on a case worked by hand, the
conditions those tests lean on -- shown from the oracle alone --, the new symbols' answers without a device and the command
line's usage errors."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bramble_amd import lib
from tests import alphabet_cases as ac
from tests import unprojected_cases as uc
from tests.test_collate_cpu import _rec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")


def test_yardstick_by_hand():
    """six records, three names: a's pair is half projected, b (three alignments) not at all, c whole"""
    recs = [_rec(b"a", 100, flag=0x41), _rec(b"a", 300, flag=0x81), _rec(b"b", 10), _rec(b"b", 20), _rec(b"b", 30), _rec(b"c", 5)]
    rows = [0, 0, 5]   # a/1 twice (two transcripts), c once
    n = len(recs[0])
    assert all(len(r) == n for r in recs) and uc.groups_of(recs) == [(0, 2), (2, 5), (5, 6)]
    s, off, st = uc.yardstick(recs, rows, "record")
    assert bytes(s) == b"".join(recs[i] for i in (1, 2, 3, 4)) and list(off) == [0, n, 2 * n, 3 * n, 4 * n]
    assert st == [6, 4, 4 * n, 3, 1, 1]
    s, off, st = uc.yardstick(recs, rows, "name")
    assert bytes(s) == b"".join(recs[i] for i in (2, 3, 4)) and list(off) == [0, n, 2 * n, 3 * n]
    assert st == [6, 3, 3 * n, 3, 1, 1]
    # every record projected: nothing; none: the input
    s, off, st = uc.yardstick(recs, list(range(6)), "record")
    assert s.size == 0 and list(off) == [0] and st == [6, 0, 0, 3, 0, 0]
    for scope in uc.SCOPES:
        s, off, st = uc.yardstick(recs, [], scope)
        assert bytes(s) == b"".join(recs) and st == [6, 6, 6 * n, 3, 3, 0]


@pytest.mark.parametrize("case", ac.BAM_CASES, ids=[c.id for c in ac.BAM_CASES])
def test_conditions_of_the_gpu_tests(case):
    """every input has unprojected records; the paired ones have partly projected names; names with no output are not the
    reference's dropped reads"""
    ann, stream, ref_map, orc, roff, rlen, recs = uc.case_input(case.id)
    assert len(recs) == len(rlen)
    _, _, st = uc.yardstick(recs, orc["input_index"], "record")
    _, _, st_name = uc.yardstick(recs, orc["input_index"], "name")
    assert st[1] >= 1 and st[0] == len(recs)
    assert st_name[1] <= st[1] and st_name[3:] == st[3:]
    if case.id in uc.PARTIAL:
        assert st[5] >= 85, st
        assert st_name[1] < st[1]
    if case.id == "adv-pe-default-22":
        assert st[4] > orc["dropped_reads"], (st[4], orc["dropped_reads"])
    if case.id in ("adv-pe-default-22", "adv-long-lr-26"):   # a reference map of all -1: no record projects
        none, _, _ = uc.oracle_bam(ann, stream, np.full(len(ref_map), -1, np.int32), case.flags)
        assert none["n_rows"] == 0


def test_new_symbols_without_a_device():
    L = lib.lib()
    L.br_ctx_unprojected_stats.argtypes = [C.c_void_p, C.c_void_p]
    L.br_ctx_unprojected_next.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.br_ctx_unprojected_reset.argtypes = [C.c_void_p]
    out, piece = (C.c_uint64 * 8)(), lib.BrDeviceBam()
    assert L.br_ctx_unprojected_stats(None, out) == -1
    assert L.br_ctx_unprojected_next(None, 1 << 20, C.byref(piece)) == -1
    assert L.br_ctx_unprojected_reset(None) == -1
    assert L.br_ctx_set_param(None, b"keep_unprojected", 1) == -1
    for name in ("br_ctx_unprojected_stats", "br_ctx_unprojected_next", "br_ctx_unprojected_reset"):
        assert name in lib.EXPORTS


def _cli(tmp_path, extra):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    return subprocess.run([BIN, str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", str(tmp_path / "o.bam")] + extra,
                          capture_output=True, timeout=60)


@pytest.mark.parametrize("extra,word", [
    (["--unprojected-scope", "name"], b"--unprojected-scope needs --unprojected"),   # the scope without the file
    (["--unprojected", "un.bam", "--unprojected-scope", "pair"], b"unknown scope pair"),   # a word other than the two
    (["--unprojected", "-"], b"standard output"),                                      # that is the main output's
    (["--unprojected", "un.bam", "--devices", "0,1"], b"--unprojected works on one device"),
])
def test_cli_usage_errors(tmp_path, extra, word):
    extra = [str(tmp_path / e) if e.endswith(".bam") else e for e in extra]
    r = _cli(tmp_path, extra)
    assert r.returncode == 2 and word in r.stderr, r.stderr.decode()
    assert sorted(os.listdir(tmp_path)) == ["g.gtf"]


def test_usage_names_the_switches():
    r = subprocess.run([BIN, "--help"], capture_output=True, timeout=60)
    assert r.returncode == 0 and b"--unprojected <unprojected.bam>" in r.stdout and b"--unprojected-scope record|name" in r.stdout
    assert b"[bramble] unprojected: R of N records written" in r.stdout

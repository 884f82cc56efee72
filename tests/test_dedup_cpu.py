"""--dedup without a GPU: the tests' restatement of br_dedup's definitions (tests/dedup_cases.py) pinned by hand -- the UMI-tools
paper's network, the count threshold, lengths, the unclipped 5' end, the signature, names without rows or without a UMI, the tag walk
-- the two formulations of the directional method against each other, the conditions the GPU tests' inputs must meet, and the new
symbols' answers without a device."""
import ctypes as C
import struct
import subprocess
from collections import Counter

import numpy as np
import pytest

from tests import bamio
from tests import dedup_cases as dc


def _mols(method, run, source="name"):
    groups = dc.records_of(run)
    umis, cnt = dc.umis_of(groups, source)
    return dc.molecules_of(method, dc.signatures_of(groups), umis), umis, cnt


def _at(umi, n, tid=0, pos=10, tag=b"x"):
    return [dc.name_row(tag + b"%d_" % j + umi, [(tid, pos, dc.cig("30M"), 0)]) for j in range(n)]


# ---- the methods -----------------------------------------------------------------------------------------------------------------
def test_the_paper_network():
    run = dc.paper_network()
    rep, umis, _ = _mols("directional", run)
    assert dc.counts_of(rep) == (623, 2, 621)
    roots = {umis[r] for r in set(rep.tolist())}
    assert roots == {b"ACGT", b"AAAT"}   # AAAT (90) is no neighbour of ACGT and 90 < 2 * 72 - 1 keeps ACAT from claiming it
    big = Counter(rep.tolist()).most_common(1)[0]
    assert umis[big[0]] == b"ACGT" and big[1] == 456 + 72 + 2 + 2 + 1   # the representative carries the most abundant UMI
    assert big[0] == min(i for i, u in enumerate(umis) if u == b"ACGT")
    assert dc.counts_of(_mols("unique", run)[0]) == (623, 6, 617)
    assert dc.hist_of(rep, 100)[100] == 1 and dc.hist_of(rep, 100)[90] == 1 and dc.hist_of(rep)[533] == 1 and dc.hist_of(rep)[0] == 0


@pytest.mark.parametrize("a,b,mols", [(3, 2, 1), (2, 2, 2), (1, 1, 1), (5, 3, 1), (5, 4, 2)])
def test_the_threshold(a, b, mols):
    run = _at(b"AAAA", a, tag=b"a") + _at(b"AAAC", b, tag=b"b")
    rep, umis, _ = _mols("directional", run)
    assert dc.counts_of(rep)[1] == mols
    if mols == 1:   # the rarer joins the more abundant; at 1 : 1 both ways, and the lower UMI is first in order
        assert set(rep.tolist()) == {0}
    assert dc.counts_of(_mols("unique", run)[0])[1] == 2


def test_lengths_and_groups_never_mix():
    run = _at(b"AAAA", 3, tag=b"a") + _at(b"AAA", 1, tag=b"b") + _at(b"AAAAC", 1, tag=b"c") + _at(b"AAAC", 1, pos=11, tag=b"d") + _at(b"AAAC", 1, tid=1, tag=b"e")
    assert dc.counts_of(_mols("directional", run)[0]) == (7, 5, 2)


def test_five():
    def five(text, pos, flag):
        return dc.entry_of(bamio.bam_record(b"r", 4, pos, dc.cig(text), 30, flag=flag))
    assert five("30M", 100, 0) == (4, 100, 0) and five("30M", 100, 16) == (4, 130, 16)
    assert five("5S25M", 100, 0)[1] == 95 and five("5S25M", 100, 16)[1] == 125
    assert five("25M5S", 100, 0)[1] == 100 and five("25M5S", 100, 16)[1] == 130
    assert five("3H4S20M6S2H", 100, 0)[1] == 96 and five("3H4S20M6S2H", 100, 16)[1] == 126
    assert five("3H20M2H", 100, 0)[1] == 100 and five("3H20M2H", 100, 16)[1] == 120   # H alone clips nothing off the coordinate
    assert five("10M100N10M2D5=3X1I4S", 100, 16)[1] == 100 + 130 + 4
    assert five("2S10M", 1, 0)[1] == -1   # signed
    assert five("30M", 100, 0x63)[2] == 0x41 and five("30M", 100, 0x193)[2] == 0x91   # paired, reverse, read1, read2 are kept
    spilled = bamio.bam_record(b"r", 4, 100, dc.cig("5S10M100N15M"), 30, flag=16, spill=True)
    assert len(bamio.record_fields(spilled)["cigar"]) == 2 and dc.entry_of(spilled) == (4, 225, 16)


def test_signature_ignores_the_order_of_the_rows():
    rows = [(3, 50, dc.cig("30M"), 0), (1, 70, dc.cig("5S25M"), 16), (3, 50, dc.cig("30M"), 0), (2, 9, dc.cig("30M"), 0x41)]
    run = [dc.name_row(b"a_ACGT", rows), dc.name_row(b"b_ACGT", rows[::-1]), dc.name_row(b"c_ACGT", rows[1:]), dc.name_row(b"d_ACGT", [])]
    sigs = dc.signatures_of(dc.records_of(run))
    assert sigs[0] == sigs[1] != sigs[2] and len(sigs[0]) == 4 and sigs[3] is None   # a multiset: the repeated entry stays
    rep, _, cnt = _mols("directional", run)
    assert list(rep) == [0, 0, 2, dc.NONE] and list(dc.dup_of(rep)) == [0, 1, 0, 0] and list(dc.groups_of(sigs)) == [0, 0, 2, dc.NONE]
    assert dc.counts_of(rep) == (4, 2, 1) and cnt["no_umi"] == 0   # the name without rows is counted nowhere


def test_names_without_a_umi():
    row = [(0, 5, dc.cig("30M"), 0)]
    run = [dc.name_row(b"plain", row), dc.name_row(b"plain2", row), dc.name_row(b"empty_", row), dc.name_row(b"long_" + b"A" * 33, row),
           dc.name_row(b"long2_" + b"A" * 33, row), dc.name_row(b"max_" + b"A" * 32, row), dc.name_row(b"a_b_AC", row)]
    rep, umis, cnt = _mols("unique", run)
    assert umis == [None] * 5 + [b"A" * 32, b"AC"] and cnt == {"no_umi": 5, "too_long": 2, "bad_aux": 0}
    assert list(rep) == list(range(7))   # never duplicates, though they share a position


def test_the_tag_walk():
    every = (b"XAAq" + b"XbcR" + b"XcC\x07" + b"XdsRR" + b"XeSRR" + b"XfiRXZ." + b"XgIRXZ." + b"XhfRXZ." + b"XiZRX\0" + b"XjH52\0" +
             b"XkBc" + struct.pack("<I", 3) + b"RXZ" + b"XlBS" + struct.pack("<I", 2) + b"RXZ." + b"XmBf" + struct.pack("<I", 1) + b"RXZ.")
    rec = bamio.bam_record(b"r", 0, 1, dc.cig("30M"), 30, aux=every + b"RXi" + struct.pack("<i", 5) + b"RXZACGT\0" + b"RXZTTTT\0")
    assert dc.umi_of_record(rec, "tag") == (b"ACGT", "")   # the first RX of type Z, behind every other type
    assert dc.umi_of_record(rec, "tag", tag=b"Xi") == (b"RX", "") and dc.umi_of_record(rec, "tag", tag=b"QQ") == (None, "none")
    assert dc.umi_of_record(rec, "name") == (None, "none")
    for bad in (b"RXZACGT", b"XXi\0\0", b"XXQ\0", b"XXBQ" + struct.pack("<I", 1) + b"\0", b"XXBi" + struct.pack("<I", 9) + b"\0" * 8, b"XX"):
        broken = bamio.bam_record(b"r", 0, 1, dc.cig("30M"), 30, aux=b"NHC\x01" + bad)
        assert dc.umi_of_record(broken, "tag") == (None, "bad_aux"), bad
    found_first = bamio.bam_record(b"r", 0, 1, dc.cig("30M"), 30, aux=b"RXZAC\0" + b"XXQ\0")
    assert dc.umi_of_record(found_first, "tag") == (b"AC", "")   # the walk ended on the UMI before it met the bad field
    assert dc.umi_of_record(bamio.bam_record(b"r", 0, 1, dc.cig("30M"), 30, aux=b"RXZ\0"), "tag") == (None, "none")
    assert dc.umi_of_record(bamio.bam_record(b"r", 0, 1, dc.cig("30M"), 30, aux=b"RXZ" + b"C" * 33 + b"\0"), "tag") == (None, "too_long")


def test_bfs_and_propagation_agree():
    rng = np.random.default_rng(5)
    differ = 0
    for k in range(200):
        n = int(rng.integers(1, 81))
        base = [dc.random_umi(rng, 6) for _ in range(max(1, n // 8))]
        counts = {}
        while len(counts) < n:
            u = base[int(rng.integers(len(base)))]
            for _ in range(int(rng.integers(0, 4))):
                u = dc.mutate(u, int(rng.integers(6)))
            if rng.integers(5) == 0:
                u = u[:5]
            counts.setdefault(u, int(rng.integers(1, 9)))
        bfs = dc.roots_by_bfs(counts)
        prop, sweeps = dc.labels_by_propagation(counts)
        assert bfs == prop and sweeps <= len(counts), k
        differ += len(set(bfs.values())) < len(counts)
    assert differ > 150   # the graphs had edges


def test_expected_stream():
    run = _at(b"AC", 2) + _at(b"GG", 1, pos=11)
    groups = dc.records_of(run)
    dup = dc.dup_of(_mols("unique", run)[0])
    assert list(dup) == [0, 1, 0]
    removed, marked = dc.expected_stream(groups, dup, False), dc.expected_stream(groups, dup, True)
    assert bytes(removed) == bytes(bamio.frame([groups[0][0], groups[2][0]]))
    got = bamio.split_stream(marked)
    assert [bamio.record_fields(r)["flag"] for r in got] == [0, 0x400, 0] and marked.size == dc.stream_of(groups).size
    diff = np.flatnonzero(marked != dc.stream_of(groups))
    assert len(diff) == 1 and diff[0] == 4 + len(groups[0][0]) + 19   # byte 19 of the second record's block: the flag word's high byte


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", [False, True])
def test_the_standard_input_meets_its_conditions(tag):
    run = dc.standard_run(tag=tag)
    groups = dc.records_of(run, spill_every=7)
    umis, cnt = dc.umis_of(groups, "tag" if tag else "name")
    sigs = dc.signatures_of(groups)
    directional, unique = dc.molecules_of("directional", sigs, umis), dc.molecules_of("unique", sigs, umis)
    n, mols, dups = dc.counts_of(directional)
    assert dups >= 0.3 * n   # at least 30 % duplicates
    by_group = {}
    for s, u in zip(sigs, umis):
        if s is not None and u is not None:
            by_group.setdefault(s, set()).add(u)
    sizes = Counter(len(v) for v in by_group.values())
    assert all(sizes[m] >= 1 for m in (1, 2, 63, 64, 65, 257)), sizes   # a group of every size around the tiles
    assert any(not np.array_equal(directional[[i for i, s in enumerate(sigs) if s == g]], unique[[i for i, s in enumerate(sigs) if s == g]]) for g in by_group)
    dup = dc.dup_of(directional)
    assert any(d and len({e[0] for e in s}) > 1 for d, s in zip(dup, sigs) if s is not None)   # a multi-transcript name among the duplicates
    rows = Counter(len(g) for g in groups)
    assert all(rows[k] >= 2 for k in (0, 1, 2, 16, 17, 64, 65, 200)), rows   # names around the lane / wave threshold, and long ones
    assert any(d and len(s) == 200 for d, s in zip(dup, sigs) if s is not None)
    if not tag:
        assert cnt["no_umi"] > 0 and cnt["too_long"] > 0
    chain = Counter(u for nm, u in zip(run, umis) if nm["name"].startswith(b"chain"))
    assert len(chain) == 96 and dc.labels_by_propagation(chain)[1] - 1 >= 95   # the chain needs at least 95 sweeps that change something
    tb = dc.tables_of(run)
    minus = [(t, p, tuple(o)) for nm in run for t, p, o, f in nm["rows"] if dc.minus_row(t, p) and o != o[::-1] and (o[0] & 15) in (4, 5)]
    assert len(minus) > 20 and np.count_nonzero(tb["a"][:, 2] & dc.ROW_MINUS) > 100   # rows whose clips change sides between row and record
    assert len(tb["a"]) == sum(len(g) for g in groups) == int(tb["row_off"][-1]) and len(tb["group_off"]) == len(run) + 1
    assert (tb["a"][:, 2] & 0xffffff).max() > 2 and sum(b"CGBI" in r for g in groups for r in g) > 10


def test_chain_is_a_path():
    for n in (1, 2, 33, 96, 97):
        counts = Counter(dc.umis_of(dc.records_of(dc.chain(n)))[0])
        adj = dc.adjacency(counts)
        assert len(counts) == n and sum(len(v) for v in adj.values()) == 2 * (n - 1)
        root, sweeps = dc.labels_by_propagation(counts)
        assert len(set(root.values())) == 1 and sweeps == max(n, 1)


# ---- the library without a device ----------------------------------------------------------------------------------------------------
SYMBOLS = ["br_dedup_new", "br_dedup_set_param", "br_dedup_add", "br_dedup_add_last", "br_dedup_finish", "br_dedup_umis", "br_dedup_result",
           "br_dedup_hist", "br_dedup_flags", "br_dedup_next", "br_dedup_stats", "br_dedup_free", "br_quant_drop_names"]


def test_new_symbols_without_a_device():
    from bramble_amd import lib
    L = lib.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_dedup_new.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.br_dedup_set_param.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.br_dedup_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    L.br_dedup_add_last.argtypes = [C.c_void_p, C.c_void_p]
    L.br_dedup_finish.argtypes = [C.c_void_p] * 4
    L.br_dedup_umis.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    L.br_dedup_result.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.br_dedup_hist.argtypes = [C.c_void_p] * 2
    L.br_dedup_flags.argtypes = [C.c_void_p] * 3
    L.br_dedup_next.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
    L.br_dedup_stats.argtypes = [C.c_void_p] * 2
    L.br_dedup_free.argtypes = [C.c_void_p]
    L.br_quant_drop_names.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    h = C.c_void_p()
    assert L.br_dedup_new(4096, C.byref(h)) == -2 and not h.value   # BR_ERR_NO_DEVICE
    assert L.br_dedup_new(0, None) == -1
    rows, recs, piece = lib.BrDeviceRows(), lib.BrDeviceBam(), lib.BrDeviceBam()
    assert L.br_dedup_set_param(None, b"method", 1) == -1 and L.br_dedup_add(None, C.byref(recs), C.byref(rows), None, 0, 0, None) == -1   # BR_ERR_INVALID_ARG
    assert L.br_dedup_add_last(None, None) == -1 and L.br_dedup_finish(None, None, None, None) == -1
    assert L.br_dedup_umis(None, 0, 0, None, None) == -1 and L.br_dedup_result(None, 0, 0, None, None, None) == -1
    assert L.br_dedup_hist(None, None) == -1 and L.br_dedup_flags(None, None, None) == -1 and L.br_dedup_next(None, 1, C.byref(piece)) == -1
    assert L.br_dedup_stats(None, None) == -1 and L.br_quant_drop_names(None, None, 0, 0, None) == -1
    L.br_dedup_free(None)
    for name in ("add_host", "add_device", "add_last", "finish", "umis", "result", "hist", "pieces", "next_records", "stats", "_raw"):
        assert hasattr(lib.Dedup, name), name
    assert hasattr(lib.Quant, "drop_names")


@pytest.mark.parametrize("extra,word", [
    (["--dedup-stats", "s.tsv"], b"need --dedup"),
    (["--dedup-umi", "tag"], b"need --dedup"),
    (["--dedup", "both"], b"unknown method both"),
    (["--dedup", "unique", "--dedup-umi-sep", "__"], b"is not one character"),
    (["--dedup", "unique", "--dedup-umi-tag", "R"], b"is not a two-character tag"),
    (["--dedup", "unique", "--dedup-bam-mode", "mark"], b"--dedup-bam-mode needs --dedup-bam"),
    (["--dedup", "unique", "--dedup-bam", "-"], b"--dedup-bam needs a file"),
    (["--dedup", "unique", "--devices", "0,1"], b"--dedup works on one device"),
    (["--dedup", "directional", "--quant", "q.tsv", "--quant-bam", "p.bam"], b"--dedup not with --quant-bam: the posterior BAM needs a class"),
    (["--dedup", "directional", "--quant", "q.tsv", "--coverage", "c.bg", "--coverage-weight", "em"], b"--dedup not with --coverage-weight em"),
])
def test_usage_errors(tmp_path, extra, word):
    import os
    from tests.test_gpu_collate import BIN
    r = subprocess.run([BIN, "in.bam", "-G", "g.gtf", "-o", "o.bam"] + extra, capture_output=True, cwd=str(tmp_path), timeout=60)
    assert r.returncode != 0 and word in r.stderr, r.stderr[:300]
    assert os.listdir(str(tmp_path)) == []

"""--quant-eff-length on the GPU: br_quant's fragment-length histogram, its three counters and the effective lengths against the
tests' restatement of the definitions (test_quant_fld_cpu.py) on the oracle's rows of the synthetic inputs -- fed from the host,
from HBM and from a context's last projection call -- and on a hand-built table for what those inputs barely touch; the EM over
1 / effective length under the rule of test_gpu_quant; the errors; and the command line with the two switches."""
import functools
import os

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests.test_gpu_collate import _coordinate_stream, _files, _inputs, _report, _run
from tests.test_gpu_quant import _assert_em, _body, _fill, _new, _rows_a
from tests.test_quant_cpu import classes_of, parse_eq_classes, unique_ambig
from tests.test_quant_fld_cpu import (LEAD, ROW_FIRST, ROW_MINUS, ROW_PAIRED, ROW_SAME_TX, eff_lengths, fragments_of, packed_of, rows_of,
                                      wide_rows)

pytestmark = pytest.mark.gpu

SIDE = ("n_obs", "n_no_fragment", "n_out_of_range")


@functools.lru_cache(maxsize=None)
def _tables(mode):
    """(oracle_tables, the oracle's rows, the same as packed device rows, the yardstick's histogram at the default fld_max)"""
    tb, rows = wide_rows(mode)
    return tb, rows, packed_of(rows), fragments_of(rows, tb["row_off"], tb["group_off"], 1000)


def _cuts(n_groups, calls):
    return [0, n_groups] if calls == 1 else [0, n_groups // 3, n_groups // 3 + 1, n_groups]   # (a call of one name among them)


def _fill_rows(q, pk, row_off, group_off, how):
    """the whole row table into `q`: from host memory or from HBM, in 1 or 3 calls"""
    import torch
    a, ref, pool = pk
    n_groups = len(group_off) - 1
    cuts = _cuts(n_groups, 3 if how.endswith("3") else 1)
    if how.startswith("host"):
        for g0, g1 in zip(cuts, cuts[1:]):
            q.add_rows_host(a, ref, pool, row_off, group_off[g0:g1 + 1])
        return
    d_a = torch.from_numpy(a.view(np.int32)).cuda()
    d_ref = torch.from_numpy(ref.view(np.int64)).cuda()
    d_pool = torch.from_numpy(pool.view(np.int32)).cuda()
    d_ro = torch.from_numpy(np.asarray(row_off, dtype=np.uint64).view(np.int64)).cuda()
    d_go = torch.from_numpy(np.asarray(group_off, dtype=np.uint32).view(np.int32)).cuda()
    for g0, g1 in zip(cuts, cuts[1:]):
        q.add_rows_device(d_a, d_ref, d_pool, d_ro, d_go, g0, g1)


def _assert_fld(got, want, tag=""):
    assert {k: got[k] for k in SIDE} == {k: want[k] for k in SIDE}, tag
    assert np.array_equal(got["hist"], want["hist"]), tag
    assert got["n_obs"] == int(got["hist"].sum())


def _same_bits(x, y):
    return np.array_equal(np.asarray(x, dtype=np.float64).view(np.uint64), np.asarray(y, dtype=np.float64).view(np.uint64))


# ---- the histogram on the synthetic inputs ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how", ["host", "host3", "dev1", "dev3", "last_batch", "last_resident"])
def test_histogram_matches_the_yardstick(mode, how):
    tb, _, pk, want = _tables(mode)
    q = _new(tb, eff_len=1)
    if how.startswith("last"):
        _fill(q, tb, how)   # (br_quant_add_last hands the context's whole row table over)
    else:
        _fill_rows(q, pk, tb["row_off"], tb["group_off"], how)
    _assert_fld(q.fld(), want, how)
    if mode == "ont":
        assert not q.fld()["hist"].any() and want["n_no_fragment"] > 100
    else:
        assert want["n_obs"] >= 300
    q.finish()
    _assert_fld(q.fld(), want, how)
    assert _same_bits(q.eff_lengths(), eff_lengths(want["hist"], tb["lens"], 1000))
    q.close()


# ---- a hand-built table ------------------------------------------------------------------------------------------------------------
N_BULK = 100000


@functools.lru_cache(maxsize=None)
def _hand_built(fld_max):
    """What the synthetic input barely touches: pooled CIGARs of 3, 64, 65 and 300 ops over the whole alphabet (the leader's, the
    mate's, both); names of 16, 17, 40 and 150 rows whose first fragment is their last two rows; a large name with two fragments,
    one without any, an ambiguous one; a leader that is its name's last row in front of a name that begins like a mate; a neighbour
    that is not paired, one on another transcript; an ambiguous name with a fragment; a name without rows; lengths 0, fld_max and
    fld_max + 1; and N_BULK unique names of one length.  -> (rows, row_off, group_off, lengths per transcript)"""
    rng = np.random.RandomState(7)
    lead, mate = LEAD, ROW_PAIRED | ROW_SAME_TX

    def wide(n):   # n ops, every op code 0 .. 8 in turn, 1 .. 3 bases each
        return [((1 + int(rng.randint(3))) << 4) | (k % 9) for k in range(n)]

    def tail(tid, n_rows, a, b):   # n_rows rows on `tid`: unpaired ones, then the fragment (a, b)
        return [(tid, k, ROW_FIRST, "10M") for k in range(n_rows - 2)] + [(tid, 100, lead, a), (tid, 50, mate | ROW_MINUS, b)]
    names = []
    for i, n in enumerate((3, 64, 65, 300)):
        names.append([(10 + i, 5, lead, wide(n)), (10 + i, 9, mate, "30M")])
        names.append([(10 + i, 9, lead | ROW_MINUS, "3S30M"), (10 + i, 2, mate, wide(n))])
    names.append([(14, 5, lead, wide(300)), (14, 1, mate, wide(70))])
    for tid, n_rows in ((20, 16), (21, 17), (22, 40), (23, 150)):
        names.append(tail(tid, n_rows, "25M3D25M", "40M"))
    names.append(tail(24, 129, wide(300), wide(65)))
    names.append([(25, 0, lead, "40M"), (25, 60, mate, "40M")] + tail(25, 30, "90M", "5M"))          # the first of two fragments
    names.append([(26, k, ROW_FIRST, "10M") for k in range(70)])                                      # large, no fragment
    names.append(tail(27, 40, "30M", "30M") + [(28, 0, ROW_FIRST, "10M")])                            # large, two labels
    names.append([(29, k, ROW_FIRST, "10M") for k in range(20)] + [(29, 7, lead, "30M")])             # large, the leader is the last row
    names.append([(30, 10, ROW_FIRST, "20M"), (30, 10, lead, "20M")])                                 # the leader is the last row ...
    names.append([(30, 100, mate, "20M")])                                                            # ... and the next name begins like a mate
    names.append([(31, 0, lead, "20M"), (31, 50, ROW_SAME_TX, "20M")])                                # the neighbour is not paired
    names.append([(32, 0, lead, "20M"), (33, 50, mate, "20M")])                                       # ... is on another transcript
    names.append([(34, 0, lead, "20M"), (34, 50, mate, "20M"), (35, 0, ROW_FIRST, "20M")])            # ambiguous, with a fragment
    names.append([])
    names.append([(36, 7, lead, []), (36, 7, mate, "4S")])                                            # length 0
    names.append([(37, 0, lead, "%dM" % fld_max), (37, 3, mate, "1M")])                               # fld_max
    names.append([(37, 4, lead, "1M"), (37, 3 + fld_max, mate, "1=")])                                # fld_max, from the positions
    names.append([(38, 0, lead, "%dM" % (fld_max + 1)), (38, 3, mate, "1M")])                         # fld_max + 1
    for j in range(N_BULK):
        names.append([(40 + j % 50, 100, lead, "12M"), (40 + j % 50, 110, mate, "12M")])              # 22
    rows = rows_of([item for nm in names for item in nm])
    row_off, group_off = [0], [0]
    for nm in names:   # every name is two alignments; the first leads all the rows
        row_off += [row_off[-1] + len(nm), row_off[-1] + len(nm)]
        group_off.append(group_off[-1] + 2)
    lens = rng.randint(1, 3000, size=100).astype(np.int64)
    lens[:8] = [5, 21, 22, 23, fld_max, fld_max + 1, 70000, 1]
    lens[90:] = [0, -1, 0, -7, 0, 0, 0, 0, 0, 0]
    return rows, np.asarray(row_off, dtype=np.uint64), np.asarray(group_off, dtype=np.uint32), lens


@pytest.mark.parametrize("fld_max", [37, 1000, 65535])
def test_hand_built_table(fld_max):
    rows, row_off, group_off, lens = _hand_built(fld_max)
    want = fragments_of(rows, row_off, group_off, fld_max)
    print("fld_max %d: %d observations in %d bins, %d unique names without a fragment, %d out of range"
          % (fld_max, want["n_obs"], int(np.count_nonzero(want["hist"])), want["n_no_fragment"], want["n_out_of_range"]))
    assert want["hist"][22] == N_BULK and want["hist"][fld_max] >= 2 and want["n_no_fragment"] == 5
    assert want["n_out_of_range"] >= 2 and (fld_max < 1000 or want["n_out_of_range"] == 2)
    assert fld_max < 1000 or int(np.count_nonzero(want["hist"])) >= 8
    pk = packed_of(rows)
    eff_want = eff_lengths(want["hist"], lens, fld_max)
    for how in ("host", "dev3"):
        q = lib.Quant(len(lens), lens)
        q.set_param("eff_len", 1)
        q.set_param("fld_max", fld_max)
        _fill_rows(q, pk, row_off, group_off, how)
        _assert_fld(q.fld(), want, how)
        q.finish()
        assert q.n_names == len(group_off) - 1
        assert _same_bits(q.eff_lengths(), eff_want), how
        q.close()
    assert np.all(eff_want[:90] >= 1.0) and not eff_want[90:].any()


def test_pool_reference_out_of_bounds_adds_nothing():
    import torch
    rows, row_off, group_off, lens = _hand_built(1000)
    n_small = len(group_off) - 1 - N_BULK
    group_off = group_off[:n_small + 1]            # (the names in front of the bulk are enough here)
    a, ref, pool = packed_of(rows)
    want = fragments_of(rows, row_off, group_off, 1000)
    big = int(np.flatnonzero((a[:, 2] & 0xffffff) == 300)[0])          # the first CIGAR of 300 ops: a small name's leader
    wave = int(np.flatnonzero((a[:, 0] == 24) & ((a[:, 2] & 0xffffff) == 300))[0])   # the one a wave sums in the large name
    for row, off in ((big, len(pool) - 299), (big, 1 << 40), (wave, len(pool) - 299), (wave, len(pool) + 1)):
        bad = ref.copy()
        bad[row] = off
        q = lib.Quant(len(lens), lens)
        q.set_param("eff_len", 1)
        rc = q.add_rows_raw(a.ctypes.data, bad.ctypes.data, pool.ctypes.data, row_off.ctypes.data, len(a), len(pool), group_off.ctypes.data,
                            n_small, False)
        assert rc == -1, (row, off)
        got = q.fld()
        assert not got["hist"].any() and [got[k] for k in SIDE] == [0, 0, 0]
        q.add_rows_host(a, ref, pool, row_off, group_off)               # the good table, then the bad one once more, from HBM
        d = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), bad.view(np.int64), pool.view(np.int32), row_off.view(np.int64),
                                                  group_off.view(np.int32))]
        rc = q.add_rows_raw(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), len(a), len(pool), d[4].data_ptr(), n_small,
                            True, torch.cuda.current_stream().cuda_stream)
        assert rc == -1, (row, off)
        _assert_fld(q.fld(), want)
        assert q.finish()[0] == n_small
        q.close()
    # rows past n_rows are refused as well
    q = lib.Quant(len(lens), lens)
    q.set_param("eff_len", 1)
    assert q.add_rows_raw(a.ctypes.data, ref.ctypes.data, pool.ctypes.data, row_off.ctypes.data, int(row_off[int(group_off[-1])]) - 1, len(pool),
                          group_off.ctypes.data, n_small, False) == -1
    q.close()


def test_a_refused_add_fixes_the_parameters():
    """The histogram's tables are sized by the first add that counts fragments, refused or not: "fld_max" and "eff_len" are
    refused from then on, and the adds that follow count into a table of the size that add saw."""
    L = lib.lib()
    rows, row_off, group_off, lens = _hand_built(1000)
    n_small = len(group_off) - 1 - N_BULK
    group_off = group_off[:n_small + 1]
    a, ref, pool = packed_of(rows)
    want = fragments_of(rows, row_off, group_off, 1000)
    bad = ref.copy()
    bad[int(np.flatnonzero((a[:, 2] & 0xffffff) == 300)[0])] = len(pool)
    q = lib.Quant(len(lens), lens)
    q.set_param("eff_len", 1)
    assert q.add_rows_raw(a.ctypes.data, bad.ctypes.data, pool.ctypes.data, row_off.ctypes.data, len(a), len(pool), group_off.ctypes.data,
                          n_small, False) == -1
    assert L.br_quant_set_param(q.h, b"fld_max", 65535) == -1 and L.br_quant_set_param(q.h, b"fld_max", 37) == -1
    assert L.br_quant_set_param(q.h, b"eff_len", 0) == -1
    _fill_rows(q, (a, ref, pool), row_off, group_off, "dev3")
    _assert_fld(q.fld(), want)
    assert q.finish()[0] == n_small
    assert _same_bits(q.eff_lengths(), eff_lengths(want["hist"], lens, 1000))
    q.close()
    # an add refused before anything was sized (no CIGARs at all) fixes nothing
    q = lib.Quant(len(lens), lens)
    q.set_param("eff_len", 1)
    assert q.add_raw(a.ctypes.data, row_off.ctypes.data, group_off.ctypes.data, n_small, False) == -1
    q.set_param("fld_max", 37)
    _fill_rows(q, (a, ref, pool), row_off, group_off, "host")
    _assert_fld(q.fld(), fragments_of(rows, row_off, group_off, 37))
    q.close()


# ---- EM ------------------------------------------------------------------------------------------------------------------------
def test_em_over_effective_lengths():
    tb, _, pk, want = _tables("pe")
    cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
    eff_want = eff_lengths(want["hist"], tb["lens"], 1000)
    results = []
    for how in ("dev1", "dev3", "dev1", "host"):
        q = _new(tb, eff_len=1, max_iters=200, tolerance=0)
        _fill_rows(q, pk, tb["row_off"], tb["group_off"], how)
        q.finish()
        assert _same_bits(q.eff_lengths(), eff_want)
        assert q.em()[0] == 200
        results.append(q.result())
        q.close()
    for other in results[1:]:   # two runs, 1-call against 3-call adds, HBM against host memory: the same bits
        for key in ("theta", "tpm"):
            assert _same_bits(results[0][key], other[key]), key
    _assert_em(results[0], cl, tb["n_tx"], eff_want, True, 200, "pe eff_len=1")
    q = _new(tb, max_iters=200, tolerance=0)
    q.add_host(_rows_a(tb["tids"]), tb["row_off"], tb["group_off"])
    q.finish()
    q.em()
    plain = q.result()
    q.close()
    short = (tb["lens"] < 400) & (plain["tpm"] > 0)
    moved = short & (plain["tpm"] != results[0]["tpm"])
    print("transcripts shorter than 400 with reads: %d, of them with another TPM under eff_len: %d" % (int(short.sum()), int(moved.sum())))
    assert moved.any()


def test_add_rows_without_the_model_is_add():
    tb, _, pk, _ = _tables("pe")
    out = []
    for how in ("plain", "host", "dev3"):
        q = _new(tb, max_iters=64, tolerance=0)
        if how == "plain":
            q.add_host(_rows_a(tb["tids"]), tb["row_off"], tb["group_off"])
        else:
            _fill_rows(q, pk, tb["row_off"], tb["group_off"], how)
        got = q.fld()
        assert not got["hist"].any() and [got[k] for k in SIDE] == [0, 0, 0]   # nothing is counted without the switch
        q.finish()
        q.em()
        out.append((q.classes(), q.result()))
        assert lib.lib().br_quant_eff_lengths(q.h, np.zeros(tb["n_tx"]).ctypes.data) == -1
        q.close()
    for (cls, res) in out[1:]:
        for x, y in zip(out[0][0], cls):
            assert np.array_equal(x, y)
        for key in ("theta", "tpm"):
            assert _same_bits(out[0][1][key], res[key]), key
        for key in ("unique", "ambig"):
            assert np.array_equal(out[0][1][key], res[key]), key


# ---- errors --------------------------------------------------------------------------------------------------------------------
def test_errors():
    L = lib.lib()
    tb, _, pk, _ = _tables("pe")
    a, ro, go = _rows_a(tb["tids"]), tb["row_off"], tb["group_off"]
    eff = np.zeros(tb["n_tx"], dtype=np.float64)
    q = _new(tb, eff_len=1)
    assert L.br_quant_set_param(q.h, b"fld_max", 0) == -1 and L.br_quant_set_param(q.h, b"fld_max", 65536) == -1
    assert L.br_quant_set_param(q.h, b"eff_len", 2) == -1
    assert q.add_raw(a.ctypes.data, ro.ctypes.data, go.ctypes.data, len(go) - 1, False) == -1   # br_quant_add has no CIGARs
    assert L.br_quant_set_param(q.h, b"fld_max", 500) == 0                                     # nothing was added yet
    q.set_param("fld_max", 1000)
    _fill_rows(q, pk, ro, go, "host")
    assert L.br_quant_set_param(q.h, b"fld_max", 500) == -1                                    # after an add
    assert L.br_quant_set_param(q.h, b"eff_len", 0) == -1
    assert L.br_quant_eff_lengths(q.h, eff.ctypes.data) == -1                                  # before finish
    q.set_param("length_norm", 0)
    q.finish()
    assert L.br_quant_em(q.h, None, None) == -1                                                # eff_len without length_norm
    assert L.br_quant_eff_lengths(q.h, eff.ctypes.data) == 0                                   # (the lengths are there)
    q.close()
    q = lib.Quant(tb["n_tx"])                                                                  # no lengths
    q.set_param("eff_len", 1)
    _fill_rows(q, pk, ro, go, "host")
    q.finish()
    assert L.br_quant_em(q.h, None, None) == -1 and L.br_quant_eff_lengths(q.h, eff.ctypes.data) == -1
    assert q.fld()["n_obs"] >= 300                                                             # the histogram does not need them
    q.close()


# ---- command line ------------------------------------------------------------------------------------------------------------------
def _parse_eff_tsv(text):
    lines = text.split("\n")
    assert lines[0] == "Name\tLength\tEffectiveLength\tNumReads\tTPM\tUniqueReads\tAmbigReads" and lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    assert all(len(f) == 7 for f in rows)
    return rows


def _fld_tsv(hist):
    return "FragmentLength\tCount\n" + "".join("%d\t%d\n" % (f, int(n)) for f, n in enumerate(hist))


def test_cli_eff_length(tmp_path):
    from tests.test_quant_cpu import parse_quant_tsv
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    sorted_bam, _ = _files(tmp_path, annd, _coordinate_stream(stream), "sorted")
    tb, rows = wide_rows("pe", guide_order=True)   # (the command line numbers the transcripts in guide order)
    want = fragments_of(rows, tb["row_off"], tb["group_off"], 1000)
    tb_col, rows_col = wide_rows("pe", guide_order=True, collated=True)
    want_col = fragments_of(rows_col, tb_col["row_off"], tb_col["group_off"], 1000)
    # (the oracle pairs the collated records of a few read names differently, so that run has yardsticks of its own)
    print("in input order: %s; collated: %s" % ([want[k] for k in SIDE], [want_col[k] for k in SIDE]))
    expect = {"eff": (tb, rows, want), "samout": (tb, rows, want), "collate": (tb_col, rows_col, want_col)}
    tx_names = [t["id"] for t in tb["annd"]["transcripts"]]

    def files(tag):
        return [str(tmp_path / ("%s.%s" % (tag, ext))) for ext in ("out", "q.tsv", "eq.txt", "fld.tsv")]
    o0, q0, c0, _ = files("plain")
    r0 = _run([in_bam, "-G", gtf, "--quant", q0, "--quant-classes", c0], o0)
    base = parse_quant_tsv(open(q0).read())
    plain = {"eff": r0, "samout": r0, "collate": _run([sorted_bam, "--collate", "-G", gtf], str(tmp_path / "plain_collate.out"))}
    text, api = {}, {}
    for tag, args in (("eff", [in_bam]), ("collate", [sorted_bam, "--collate"]), ("samout", [in_bam, "-O", "sam"])):
        tb, rows, want = expect[tag]
        if id(tb) not in api:   # the library's own result on the same rows: the floats are compared as printed
            q = _new(tb, eff_len=1)
            _fill_rows(q, packed_of(rows), tb["row_off"], tb["group_off"], "host")
            q.finish()
            q.em()
            api[id(tb)] = q.result()
            q.close()
        res = api[id(tb)]
        eff_want = eff_lengths(want["hist"], tb["lens"], 1000)
        cl = classes_of(tb["tids"], tb["row_off"], tb["group_off"])
        uniq, ambig = unique_ambig(cl, tb["n_tx"])
        o1, q1, c1, f1 = files(tag)
        r1 = _run(args + ["-G", gtf, "--quant", q1, "--quant-classes", c1, "--quant-eff-length", "--quant-fld", f1], o1)
        text[tag] = [open(p).read() for p in (q1, c1, f1)]
        got = _parse_eff_tsv(text[tag][0])
        # the table: what the switch leaves alone, and the new column as the yardstick prints it
        assert [f[0] for f in got] == tx_names == [r[0] for r in base] and [int(f[1]) for f in got] == [r[1] for r in base], tag
        assert [int(f[5]) for f in got] == uniq.tolist() and [int(f[6]) for f in got] == ambig.tolist(), tag
        if tag != "collate":
            assert [int(f[5]) for f in got] == [r[4] for r in base] and [int(f[6]) for f in got] == [r[5] for r in base], tag
        assert [f[2] for f in got] == ["%.3f" % v for v in eff_want], tag
        assert [f[3] for f in got] == ["%.6f" % v for v in res["theta"]] and [f[4] for f in got] == ["%.6f" % v for v in res["tpm"]], tag
        assert text[tag][2] == _fld_tsv(want["hist"]), tag
        # the report: one more line, in front of the quantified line; the rest is the run's without the switch
        out1 = r1.stdout.decode().split("\n")
        mean = sum(float(f) * float(n) for f, n in enumerate(want["hist"])) / float(want["n_obs"])
        line = "[bramble] fragment lengths: %d observed, mean %.1f, %d unique names without a pair, %d out of range" % (
            want["n_obs"], mean, want["n_no_fragment"], want["n_out_of_range"])
        assert out1.count(line) == 1, (tag, [l for l in out1 if "fragment" in l])
        assert out1.index(line) + 1 == next(i for i, l in enumerate(out1) if l.startswith("[bramble] quantified ")), tag
        assert _report(r1) == _report(plain[tag]) and len(_report(r1)) == 5, tag
        for p in (q1, c1, f1, o1):
            assert not os.path.exists(p + ".tmp-bramble")
    # the projected output is the run's without the switches
    h0, s0 = _body(o0, False)
    h1, s1 = _body(files("eff")[0], False)
    assert h0 == h1 and np.array_equal(s0, s1) and len(s0) > 100000
    assert not any("fragment lengths" in l for l in r0.stdout.decode().split("\n"))
    assert text["eff"][1] == open(c0).read()   # the classes do not depend on the model
    moved = [(b[1], b[3], f[4]) for b, f in zip(base, _parse_eff_tsv(text["eff"][0])) if b[1] < 400 and b[3] != f[4]]
    assert moved   # a short transcript's TPM differs
    # SAM output: the same three quant files.  --collate on the coordinate-sorted input was held to the yardsticks on the collated
    # records above; its classes are the restatement's, in the order of its read names
    assert text["samout"] == text["eff"]
    names_c, labels_c, counts_c = parse_eq_classes(text["collate"][1])
    cl = classes_of(tb_col["tids"], tb_col["row_off"], tb_col["group_off"])
    assert names_c == tx_names and labels_c == cl["labels"] and counts_c == cl["counts"]
    assert np.array_equal(want_col["hist"], expect["eff"][2]["hist"]) and text["collate"][2] == text["eff"][2]

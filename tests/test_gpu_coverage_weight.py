"""--coverage-weight on the GPU: br_quant's name classes and posteriors, and br_coverage's weighted depth (weight nh and weight em),
against the tests' restatement of the definitions (test_coverage_weight_cpu.py) on the oracle's rows of the synthetic inputs and on
hand-built tables; the carry of a 64-bit depth through the scan; the errors; the memory account; and the command line."""
import functools
import os

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests.test_coverage_weight_cpu import (NO_CLASS, ONE, name_classes_of, nh_of, posteriors_of, row_names_of, weight_words_em,
                                            weight_words_nh, weighted_coverage_of)
from tests.test_gpu_collate import _files, _inputs, _report, _run
from tests.test_gpu_quant import _batch_of, _body
from tests.test_quant_cpu import classes_of, weights
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_PAIRED, ROW_PRIMARY, packed_of, rows_of, wide_rows

pytestmark = pytest.mark.gpu

COUNTERS = ("rows_counted", "rows_skipped", "clipped_bases")
SUMMARY = ("records", "weight_sum", "aligned_hi", "aligned_lo", "covered_bases", "max_depth")


@functools.lru_cache(maxsize=None)
def _tables(mode):
    """the input's oracle tables, its rows (yardstick form and packed, nh = the rows of the row's name), and the names' yardstick"""
    tb, rows = wide_rows(mode)
    a, ref, pool = packed_of(rows)
    n_rows = len(a)
    nh = nh_of(n_rows, tb["row_off"], tb["group_off"])
    a[:, 3] = nh
    return {"tb": tb, "rows": rows, "pk": (a, ref, pool), "nh": nh, "cl": classes_of(tb["tids"], tb["row_off"], tb["group_off"]),
            "ncls": name_classes_of(tb["tids"], tb["row_off"], tb["group_off"]), "names": row_names_of(n_rows, tb["row_off"], tb["group_off"])}


def _name_cuts(n, calls):
    return [0, n] if calls == 1 else [0, n // 3, n // 3 + 1, n]   # (a call of one name among them)


def _fill_names(objs, pk, row_off, group_off, how):
    """the read names into every object of `objs` (Quant: add_rows_*, Coverage: add_names_*), call by call: from host memory ("host",
    "host3") or from HBM ("dev1", "dev3")"""
    import torch
    a, ref, pool = pk
    ro, go = np.ascontiguousarray(row_off, dtype=np.uint64), np.ascontiguousarray(group_off, dtype=np.uint32)
    cuts = _name_cuts(len(go) - 1, 3 if how.endswith("3") else 1)
    if how.startswith("dev"):
        d = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), ref.view(np.int64), pool.view(np.int32), ro.view(np.int64), go.view(np.int32))]
    for g0, g1 in zip(cuts, cuts[1:]):
        for o in objs:
            if how.startswith("host"):
                (o.add_rows_host if isinstance(o, lib.Quant) else o.add_names_host)(a, ref, pool, ro, go[g0:g1 + 1])
            else:
                (o.add_rows_device if isinstance(o, lib.Quant) else o.add_names_device)(*d, g0, g1)


def _fill_last(objs, tb):
    """the input through a context, every object taking the call's rows with add_last"""
    from bramble_amd import device
    idx = lib.Index(tb["annd"], device=0)
    ctx = lib.Context(idx)
    db = device.upload_batch(_batch_of(tb))
    ctx.project_batch_device(lib.make_config(**tb["flags"]), db)
    for o in objs:
        o.add_last(ctx)
    ctx.close()
    idx.close()


def _fill_rows(c, pk, how):
    import torch
    a, ref, pool = pk
    cuts = [0, len(a)] if not how.endswith("3") else [0, len(a) // 3, len(a) // 3 + 1, len(a)]
    if how.startswith("host"):
        for r0, r1 in zip(cuts, cuts[1:]):
            c.add_rows_host(a, ref, pool, r0, r1)
        return
    d = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), ref.view(np.int64), pool.view(np.int32))]
    for r0, r1 in zip(cuts, cuts[1:]):
        c.add_rows_device(*d, r0, r1)


def _quant(n_tx, lens, **params):
    q = lib.Quant(n_tx, lens)
    q.set_param("keep_names", 1)
    for k, v in params.items():
        q.set_param(k, v)
    return q


def _w_of(q, lens, n_tx, length_norm, eff_len):
    """the w the EM used, as bramble_amd.h documents it"""
    if eff_len:
        eff = q.eff_lengths()
        return np.where(eff > 0, 1.0 / np.where(eff > 0, eff, 1.0), 0.0)
    return weights(lens, n_tx, length_norm)


def _assert_weighted(c, want, lens, depth_of, tag=""):
    got = c.runs64()
    assert c.n_runs == len(want["runs"][0]), tag
    for g, w, name in zip(got, want["runs"], ("tid", "start", "end", "depth")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (tag, name)
    s = c.summary64()
    for k in SUMMARY:
        assert s[k].dtype == np.uint64 and np.array_equal(s[k], want[k]), (tag, k)
    st = c.stats()
    assert {k: st[k] for k in COUNTERS} == {k: want[k] for k in COUNTERS}, tag
    for t in depth_of:
        d = c.depth64(t)
        assert d.dtype == np.uint64 and len(d) == max(int(lens[t]), 0) and np.array_equal(d, want["depth"][t]), (tag, t)
    return st


def _some(want, tb):
    return sorted({int(np.argmax(want["max_depth"])), int(np.argmax(want["records"])), 0, tb["n_tx"] // 2, tb["n_tx"] - 1, int(np.argmax(tb["lens"]))})


# ---- names and posteriors --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how,bits", [("host", 64), ("dev1", 64), ("dev3", 64), ("dev3", 4), ("host", 4)])
def test_name_classes_match_the_yardstick(mode, how, bits):
    t = _tables(mode)
    tb = t["tb"]
    q = _quant(tb["n_tx"], tb["lens"], hash_bits=bits)
    _fill_names([q], t["pk"], tb["row_off"], tb["group_off"], how)
    n_names, n_classes = q.finish()
    assert n_names == len(t["ncls"]) and n_classes == len(t["cl"]["labels"])
    got = q.name_classes()
    assert got.dtype == np.uint32 and np.array_equal(got, t["ncls"]), (mode, how, bits)
    assert np.count_nonzero(t["ncls"] == NO_CLASS) >= 1 and (bits == 64 or q.stats()["collisions"] > 0)
    assert np.array_equal(q.name_classes(7, 5), t["ncls"][7:12])
    assert q._raw("name_classes", 0, n_names + 1, None) == -1 and q._raw("name_classes", -1, 1, None) == -1
    q.close()


def _assert_posteriors(q, cl, lens, n_tx, length_norm, eff_len, tag):
    """bit equality: theta is an input here, and every operation is one IEEE rounding in a fixed order"""
    theta = q.result()["theta"]
    want = posteriors_of(cl, theta, _w_of(q, lens, n_tx, length_norm, eff_len))
    got = q.posteriors()
    assert got.dtype == np.float64 and len(got) == len(want) == sum(len(s) for s in cl["labels"]), tag
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (tag, int(np.count_nonzero(got.view(np.uint64) != want.view(np.uint64))))
    return got


@pytest.mark.parametrize("mode,length_norm,eff_len", [("pe", 1, 0), ("ont", 0, 0), ("pe", 1, 1), ("ont", 1, 0)])
def test_posteriors_are_bit_equal(mode, length_norm, eff_len):
    t = _tables(mode)
    tb = t["tb"]
    q = _quant(tb["n_tx"], tb["lens"], length_norm=length_norm, eff_len=eff_len)
    assert q._raw("posteriors", None) == -1                       # before finish
    _fill_names([q], t["pk"], tb["row_off"], tb["group_off"], "dev1")
    q.finish()
    assert q._raw("posteriors", None) == -1                       # before the EM
    q.em()
    held = q.stats()["held_bytes"]
    q.posteriors(fetch=False)                                     # only made and held: 8 bytes a label, one entry more
    assert q.stats()["held_bytes"] == held + 8 * (q.stats()["n_labels"] + 1)
    post = _assert_posteriors(q, t["cl"], tb["lens"], tb["n_tx"], length_norm, eff_len, (mode, length_norm, eff_len))
    assert np.count_nonzero(post == 1.0) >= 100 and np.count_nonzero((post > 0) & (post < 1)) >= 100
    q.close()


def test_posteriors_of_wide_classes():
    """classes of 65 and of 200 labels: summed one label after the other, not by a wave's tree"""
    n_tx = 260
    rng = np.random.RandomState(11)
    names = [list(range(3, 68)), list(range(60, 260)), list(range(60, 260))] + [[int(t)] for t in rng.randint(0, n_tx, 400)] \
        + [sorted(set(int(t) for t in rng.randint(0, n_tx, 3))) for _ in range(50)]
    tids = np.asarray([t for s in names for t in s], dtype=np.uint32)
    row_off = np.concatenate([[0], np.cumsum([len(s) for s in names])]).astype(np.uint64)
    group_off = np.arange(len(names) + 1, dtype=np.uint32)
    lens = rng.randint(200, 5000, n_tx).astype(np.int64)
    cl = classes_of(tids, row_off, group_off)
    assert sorted(len(s) for s in cl["labels"])[-2:] == [65, 200]
    a = np.zeros((len(tids), 4), dtype=np.uint32)
    a[:, 0] = tids
    for length_norm in (1, 0):
        q = _quant(n_tx, lens, length_norm=length_norm)
        q.add_host(a, row_off, group_off)
        q.finish()
        q.em()
        _assert_posteriors(q, cl, lens, n_tx, length_norm, 0, length_norm)
        assert np.array_equal(q.name_classes(), name_classes_of(tids, row_off, group_off))
        q.close()


# ---- depth and tables on the synthetic inputs ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _want_nh(mode, primary_only):
    t = _tables(mode)
    return weighted_coverage_of(t["rows"], t["tb"]["lens"], weight_words_nh(t["nh"]), bool(primary_only))


@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how,primary_only", [("host", 0), ("host3", 1), ("dev1", 1), ("dev3", 0), ("names_dev3", 0)])
def test_weight_nh_matches_the_yardstick(mode, how, primary_only):
    t = _tables(mode)
    tb, want = t["tb"], _want_nh(mode, primary_only)
    done = []
    for _ in range(2):   # two runs give identical bytes
        c = lib.Coverage(tb["lens"])
        c.set_param("weight", 1)
        c.set_param("primary_only", primary_only)
        if how.startswith("names"):   # add_names is add_rows over the names' rows here
            _fill_names([c], t["pk"], tb["row_off"], tb["group_off"], how[6:])
        else:
            _fill_rows(c, t["pk"], how)
        c.finish()
        done.append(c)
    some = _some(want, tb)
    _assert_weighted(done[0], want, tb["lens"], some, (mode, how, primary_only))
    assert all(g.tobytes() == g2.tobytes() for g, g2 in zip(done[0].runs64(), done[1].runs64()))
    assert all(done[0].depth64(x).tobytes() == done[1].depth64(x).tobytes() for x in some)
    assert len(set(want["runs"][3].tolist())) > 50 and int(want["max_depth"].max()) > ONE
    for c in done:
        c.close()


@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how,primary_only", [("host", 0), ("host3", 1), ("dev1", 1), ("dev3", 0), ("last", 0)])
def test_weight_em_matches_the_yardstick(mode, how, primary_only):
    t = _tables(mode)
    tb = t["tb"]
    runs = []
    for _ in range(2):   # two runs give identical bytes
        q = _quant(tb["n_tx"], tb["lens"])
        c = lib.Coverage(tb["lens"])
        c.set_param("weight", 2)
        c.set_param("primary_only", primary_only)
        if how == "last":
            _fill_last([q, c], tb)
        else:
            _fill_names([q, c], t["pk"], tb["row_off"], tb["group_off"], how)
        q.finish()
        q.em()
        post = q.posteriors()
        c.finish_em(q)
        runs.append((c, q, post))
    (c, q, post), (c2, q2, post2) = runs
    want = weighted_coverage_of(t["rows"], tb["lens"], weight_words_em(t["cl"], post, t["ncls"], t["names"], t["rows"]["tid"]), bool(primary_only))
    some = _some(want, tb)
    _assert_weighted(c, want, tb["lens"], some, (mode, how, primary_only))
    assert np.array_equal(post.view(np.uint64), post2.view(np.uint64))
    for g, g2 in zip(c.runs64(), c2.runs64()):
        assert g.tobytes() == g2.tobytes()
    assert all(c.depth64(x).tobytes() == c2.depth64(x).tobytes() for x in some)
    assert all(np.array_equal(v, c2.summary64()[k]) for k, v in c.summary64().items())
    depths = set(want["runs"][3].tolist())
    assert len(depths) > 50 and any(0 < d < ONE for d in depths) and int(want["max_depth"].max()) > ONE
    for o in (c, q, c2, q2):
        o.close()


# ---- a hand-built table -------------------------------------------------------------------------------------------------------------
T_A, T_B, T_CLIP, T_NEXT, T_ZERO, T_AFTER, T_WIDE, T_P1, T_P2 = range(9)
HAND_LENS = np.asarray([2000, 2000, 30, 40, 0, 50, 3000, 100, 100], dtype=np.int64)
N_UNIQUE = 1000


@functools.lru_cache(maxsize=None)
def _hand_built():
    """Names (each a list of rows) for what the synthetic inputs do not hold: CIGARs on the inline path (0, 1, 2 ops), the pooled
    path (3 and 64 ops) and the wave's (65 and 300 ops), in names of several labels; an interval clipped at T_CLIP's end whose - q
    lands on T_NEXT's first base, where a row of another weight begins; T_ZERO, without bases, between covered transcripts, with a
    row on it; a pair whose mates lie on T_P1 and T_P2; N_UNIQUE names on T_A alone and one name on {T_A, T_B}, whose posterior
    on T_B the EM drives below 2^-33: a row with q == 0; names without rows."""
    rng = np.random.RandomState(3)

    def wide(n):
        return [((1 + int(rng.randint(3))) << 4) | (k % 9) for k in range(n)]
    names = [[(T_A, 10, ROW_FIRST | ROW_PRIMARY, "50M")] for _ in range(N_UNIQUE)]
    names += [[(T_A, 100, ROW_FIRST | ROW_PRIMARY, "20M"), (T_B, 100, ROW_FIRST, "20M5D20M")]]                      # q == 0 on T_B
    names += [[], []]
    names += [[(T_CLIP, 20, ROW_FIRST | ROW_PRIMARY, "25M"), (T_WIDE, 0, ROW_FIRST, wide(300))]]                     # clipped at 30
    names += [[(T_NEXT, 0, ROW_FIRST | ROW_PRIMARY, "10M")], [(T_NEXT, 0, ROW_FIRST | ROW_PRIMARY, "10M"), (T_AFTER, 0, ROW_FIRST, "10M2I5M")]]
    names += [[(T_ZERO, 0, ROW_FIRST | ROW_PRIMARY, "10M"), (T_AFTER, 40, ROW_FIRST, "10M")]]
    names += [[(T_P1, 5, ROW_PAIRED | ROW_FIRST | ROW_PRIMARY, "30M"), (T_P2, 50, ROW_PAIRED, "30M")] for _ in range(3)]
    names += [[(T_P1, 5, ROW_PAIRED | ROW_FIRST | ROW_PRIMARY, "30M"), (T_P1, 40, ROW_PAIRED, "30M")]]
    names += [[]]
    for n in (0, 1, 2, 3, 64, 65, 300):
        names += [[(T_WIDE, 100 + n, ROW_FIRST | ROW_PRIMARY, wide(n)), (T_A, 500 + n, ROW_FIRST, wide(n)), (T_B, 1990, ROW_FIRST, wide(n))]]
    names += [[(T_WIDE, 2990, ROW_FIRST | ROW_PRIMARY, wide(300))], [(T_P2, 7, ROW_FIRST | ROW_PRIMARY, "4S")], []]
    items = [r for nm in names for r in nm]
    rows = rows_of(items)
    row_off = np.concatenate([[0], np.cumsum([len(nm) for nm in names])]).astype(np.uint64)
    group_off = np.arange(len(names) + 1, dtype=np.uint32)
    return rows, row_off, group_off


def test_hand_built_table_holds_its_cases():
    rows, row_off, group_off = _hand_built()
    ops = np.diff(rows["cigar_off"].astype(np.int64))
    assert {0, 1, 2, 3, 64, 65, 300} <= set(ops.tolist())
    ncls = name_classes_of(rows["tid"], row_off, group_off)
    assert np.count_nonzero(ncls == NO_CLASS) == 4
    cov = weighted_coverage_of(rows, HAND_LENS, [ONE] * len(rows["tid"]))
    assert cov["clipped_bases"] > 15 and int(cov["records"][T_ZERO]) == 1 and cov["depth"][T_CLIP][29] == ONE and cov["depth"][T_NEXT][0] == 2 * ONE


@pytest.mark.parametrize("how", ["host", "dev3"])
@pytest.mark.parametrize("primary_only", [0, 1])
def test_hand_built_table_weight_em(how, primary_only):
    rows, row_off, group_off = _hand_built()
    pk = packed_of(rows)
    n_tx = len(HAND_LENS)
    cl = classes_of(rows["tid"], row_off, group_off)
    q = _quant(n_tx, HAND_LENS, length_norm=0)
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 2)
    c.set_param("primary_only", primary_only)
    _fill_names([q, c], pk, row_off, group_off, how)
    q.finish()
    q.em()
    post = _assert_posteriors(q, cl, HAND_LENS, n_tx, 0, 0, how)
    ncls = name_classes_of(rows["tid"], row_off, group_off)
    assert np.array_equal(q.name_classes(), ncls)
    qs = weight_words_em(cl, post, ncls, row_names_of(len(rows["tid"]), row_off, group_off), rows["tid"])
    assert qs[N_UNIQUE + 1] == 0 and qs[N_UNIQUE] == ONE and qs[0] == ONE   # the row with q == 0, beside its name's other row
    assert len(set(qs)) > 6
    want = weighted_coverage_of(rows, HAND_LENS, qs, bool(primary_only))
    c.finish_em(q)
    _assert_weighted(c, want, HAND_LENS, range(n_tx), (how, primary_only))
    if not primary_only:
        assert int(want["records"][T_B]) >= 8 and int(want["weight_sum"][T_B]) == 0 and want["depth"][T_NEXT][0] > ONE   # records of weight 0
    q.close()
    c.close()


@pytest.mark.parametrize("how", ["host", "dev3"])
def test_hand_built_table_weight_nh(how):
    rows, row_off, group_off = _hand_built()
    a, ref, pool = packed_of(rows)
    rng = np.random.RandomState(9)
    a[:, 3] = rng.choice([1, 2, 3, 5, 7, 12, 4000000000], len(a))
    want = weighted_coverage_of(rows, HAND_LENS, weight_words_nh(a[:, 3]))
    assert {1, ONE} <= set(weight_words_nh(a[:, 3]))
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 1)
    _fill_rows(c, (a, ref, pool), how)
    c.finish()
    _assert_weighted(c, want, HAND_LENS, range(len(HAND_LENS)), how)
    c.close()


# ---- the scan's carry -------------------------------------------------------------------------------------------------------------
def test_a_64_bit_depth_carried_through_more_tiles_than_one_scan_block_takes():
    """4 300 000 bases are 1 050 tiles of 4 096; five rows of NH 3 cover them, so the word carried from tile to tile is
    5 * 1431655765 = 7158278825: above bit 32"""
    lens = np.asarray([4300000, 7], dtype=np.int64)
    rows = rows_of([(0, 0, 0, "4300000M")] * 4 + [(0, 1, 0, "4299998M"), (0, 4299000, 0, "1000M"), (1, 0, 0, "7M")])
    a, ref, pool = packed_of(rows)
    a[:, 3] = 3
    want = weighted_coverage_of(rows, lens, weight_words_nh(a[:, 3]))
    q3 = 1431655765
    assert [tuple(int(v[k]) for v in want["runs"]) for k in range(len(want["runs"][0]))] == [
        (0, 0, 1, 4 * q3), (0, 1, 4299000, 5 * q3), (0, 4299000, 4299999, 6 * q3), (0, 4299999, 4300000, 5 * q3), (1, 0, 7, q3)]
    assert 5 * q3 > ONE and int(want["aligned_hi"][0]) == 4300000 and int(want["aligned_lo"][0]) > 1 << 40
    c = lib.Coverage(lens)
    c.set_param("weight", 1)
    c.add_rows_host(a, ref, pool)
    c.finish()
    _assert_weighted(c, want, lens, [0, 1])
    c.close()


# ---- errors ---------------------------------------------------------------------------------------------------------------------------
def test_errors():
    L = lib.lib()
    rows, row_off, group_off = _hand_built()
    pk = packed_of(rows)
    a, ref, pool = pk
    n_tx = len(HAND_LENS)
    out = np.zeros(4096, dtype=np.uint64)
    n = lib.C.c_int64()

    def raw_names(c, go):
        return c.add_names_raw(a.ctypes.data, ref.ctypes.data, pool.ctypes.data, row_off.ctypes.data, len(a), len(pool), go.ctypes.data, len(go) - 1, False)
    # the parameter
    c = lib.Coverage(HAND_LENS)
    assert c._raw("set_param", b"weight", 3) == -1 and c._raw("set_param", b"weight", -1) == -1
    # mode 0: add_names is add_rows; the 64-bit getters and finish_em refuse
    assert raw_names(c, group_off) == 0 and c._raw("set_param", b"weight", 1) == -1   # (after the first add)
    q = _quant(n_tx, HAND_LENS, length_norm=0)
    _fill_names([q], pk, row_off, group_off, "host")
    q.finish()
    q.em()
    assert c._raw("finish_em", q.h, lib.C.byref(n)) == -1
    c.finish()
    assert c._raw("runs64", 0, 0, None, None, None, None) == -1 and c._raw("depth64", 0, out.ctypes.data) == -1
    assert c._raw("summary64", out.ctypes.data, None, None, None, None, None) == -1
    assert c.runs()[0].size == c.n_runs > 0
    c.close()
    # mode 1: finish_em and the 32-bit getters refuse; nh == 0 is skipped and finish refuses
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 1)
    c.add_rows_host(a, ref, pool)
    assert c._raw("finish_em", q.h, lib.C.byref(n)) == -1
    c.finish()
    assert c._raw("runs", 0, 0, None, None, None, None) == -1 and c._raw("depth", 0, out.ctypes.data) == -1
    assert c._raw("summary", out.ctypes.data, None, None, None) == -1
    assert c.stats()["rows_counted"] == len(a)
    c.close()
    zero = a.copy()
    zero[5, 3] = 0
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 1)
    c.add_rows_host(zero, ref, pool)
    st = c.stats()
    assert (st["rows_counted"], st["rows_skipped"]) == (len(a) - 1, 1) and c._raw("finish", lib.C.byref(n)) == -1
    c.close()
    # mode 2: add_rows and finish refuse; finish_em wants a quantifier with keep_names, after its EM, with the same names -- and the
    # object stays usable after every refusal
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 2)
    assert c.add_rows_raw(a.ctypes.data, ref.ctypes.data, pool.ctypes.data, len(a), len(pool), 0, len(a), False) == -1
    bad = group_off.copy()
    bad[3] = bad[5]                                                         # offsets that descend: nothing is added
    assert raw_names(c, bad) == -1 and c.stats()["rows_counted"] == 0
    assert raw_names(c, group_off) == 0
    assert c._raw("finish", lib.C.byref(n)) == -1
    plain = lib.Quant(n_tx, HAND_LENS)                                      # without keep_names
    plain.set_param("length_norm", 0)
    _fill_names([plain], pk, row_off, group_off, "host")
    plain.finish()
    plain.em()
    assert plain._raw("name_classes", 0, 1, out.ctypes.data) == -1 and c._raw("finish_em", plain.h, lib.C.byref(n)) == -1
    plain.close()
    early = _quant(n_tx, HAND_LENS, length_norm=0)                           # before its EM, and before its finish
    _fill_names([early], pk, row_off, group_off, "host")
    assert c._raw("finish_em", early.h, lib.C.byref(n)) == -1
    early.finish()
    assert c._raw("finish_em", early.h, lib.C.byref(n)) == -1
    early.close()
    fewer = _quant(n_tx, HAND_LENS, length_norm=0)                           # another name count
    fewer.add_rows_host(a, ref, pool, row_off, group_off[:-1])
    fewer.finish()
    fewer.em()
    assert c._raw("finish_em", fewer.h, lib.C.byref(n)) == -1
    fewer.close()
    assert c._raw("finish_em", None, lib.C.byref(n)) == -1
    assert c._raw("runs64", 0, 0, None, None, None, None) == -1              # before finish
    cl = classes_of(rows["tid"], row_off, group_off)
    ncls = name_classes_of(rows["tid"], row_off, group_off)
    qs = weight_words_em(cl, q.posteriors(), ncls, row_names_of(len(a), row_off, group_off), rows["tid"])
    c.finish_em(q)                                                           # the refusals changed nothing
    _assert_weighted(c, weighted_coverage_of(rows, HAND_LENS, qs), HAND_LENS, range(n_tx))
    assert c._raw("finish_em", q.h, lib.C.byref(n)) == -1                    # after finish
    assert c._raw("runs", 0, 0, None, None, None, None) == -1
    c.close()
    q.close()


# ---- memory ---------------------------------------------------------------------------------------------------------------------------
def test_held_bytes_follow_the_device_memory_account():
    """coverage.cpp's account of the weighted modes, to the byte"""
    rows, row_off, group_off = _hand_built()
    pk = packed_of(rows)
    a, ref, pool = pk
    T, B = len(HAND_LENS), int(np.maximum(HAND_LENS, 0).sum())
    from_weight = 8 * (B + 1) + 24 * (T + 1) + 128
    want = weighted_coverage_of(rows, HAND_LENS, [ONE] * len(a))
    tiles = (B + 4095) // 4096
    # weight nh
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 1)
    assert c.stats()["held_bytes"] == from_weight
    c.add_rows_host(a, ref, pool)
    st = c.stats()
    assert st["held_bytes"] == from_weight and st["peak_bytes"] >= from_weight + 24 * (len(a) + 1) + 4 * (len(pool) + 1)
    n_runs = c.finish()
    assert c.stats()["held_bytes"] == from_weight + 32 * (T + 1) + 24 * (n_runs + 1)
    c.close()
    # weight em: while keeping, and after finish_em
    q = _quant(T, HAND_LENS, length_norm=0)
    c = lib.Coverage(HAND_LENS)
    c.set_param("weight", 2)
    assert c.stats()["held_bytes"] == from_weight
    _fill_names([q, c], pk, row_off, group_off, "host")
    E = want["n_entries"]
    assert c.stats()["held_bytes"] == from_weight + 16 * (E + 1)
    names = len(group_off) - 1
    q.finish()
    held_q = q.stats()["held_bytes"]
    q.em()
    q.posteriors(fetch=False)
    n_runs = c.finish_em(q)
    assert c.stats()["held_bytes"] == from_weight + 32 * (T + 1) + 24 * (n_runs + 1)
    assert c.stats()["peak_bytes"] >= from_weight + 16 * (E + 1) + 8 * (tiles + 2)
    # the quantifier: 4 bytes a name from finish on, 8 a label for the posteriors
    plain = lib.Quant(T, HAND_LENS)
    plain.set_param("length_norm", 0)
    _fill_names([plain], pk, row_off, group_off, "host")
    plain.finish()
    assert held_q == plain.stats()["held_bytes"] + 4 * (names + 1)
    for o in (q, c, plain):
        o.close()


# ---- command line ---------------------------------------------------------------------------------------------------------------------
def _bedgraph64(runs, names):
    return "".join("%s\t%d\t%d\t%.10g\n" % (names[int(t)], s, e, int(d) / 4294967296.0) for t, s, e, d in zip(*runs))


def _summary64(s, names, lens):
    out = ["Name\tLength\tRecords\tWeightedRecords\tAlignedBases\tCoveredBases\tMaxDepth\tMeanDepth\tBreadth"]
    for t in range(len(lens)):
        if lens[t] <= 0:
            continue
        aligned = float(int(s["aligned_hi"][t])) + int(s["aligned_lo"][t]) / 4294967296.0
        out.append("%s\t%d\t%d\t%.6f\t%.6f\t%d\t%.6f\t%.6f\t%.6f" % (names[t], lens[t], s["records"][t], int(s["weight_sum"][t]) / 4294967296.0, aligned,
                                                                   s["covered_bases"][t], int(s["max_depth"][t]) / 4294967296.0,
                                                                   aligned / float(lens[t]), int(s["covered_bases"][t]) / float(lens[t])))
    return "\n".join(out) + "\n"


def test_cli_coverage_weight(tmp_path):
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    tb, _ = wide_rows("pe", guide_order=True)   # (the command line numbers the transcripts in guide order)
    names = [t["id"] for t in tb["annd"]["transcripts"]]

    def paths(tag):
        return [str(tmp_path / ("%s.%s" % (tag, ext))) for ext in ("out", "bedgraph", "cov.tsv", "q.tsv")]
    base = [in_bam, "-G", gtf]
    o0, bed0, tsv0, q0 = paths("plain")
    r0 = _run(base + ["--quant", q0, "--coverage", bed0, "--coverage-summary", tsv0], o0)
    # unit: the files and the report line of the run without the switch
    o1, bed1, tsv1, q1 = paths("unit")
    r1 = _run(base + ["--quant", q1, "--coverage", bed1, "--coverage-summary", tsv1, "--coverage-weight", "unit"], o1)
    assert open(bed1, "rb").read() == open(bed0, "rb").read() and open(tsv1, "rb").read() == open(tsv0, "rb").read() and len(open(bed0).read()) > 100000
    line0 = [l for l in r0.stdout.decode().split("\n") if l.startswith("[bramble] coverage")]
    line1 = [l for l in r1.stdout.decode().split("\n") if l.startswith("[bramble] coverage")]
    assert len(line0) == len(line1) == 1 and line0[0].split(" (add ")[0] == line1[0].split(" (add ")[0] and line0[0].startswith("[bramble] coverage: ")
    h0, s0 = _body(o0, False)
    for word, weight in (("nh", 1), ("em", 2)):
        # the API's tables, from the same rows: a context's projection of the input, taken with add_last
        q = _quant(tb["n_tx"], tb["lens"])
        c = lib.Coverage(tb["lens"])
        c.set_param("weight", weight)
        _fill_last([q, c], tb)
        q.finish()
        q.em()
        if weight == 2:
            c.finish_em(q)
        else:
            c.finish()
        o, bed, tsv, qt = paths(word)
        r = _run(base + ["--quant", qt, "--coverage", bed, "--coverage-summary", tsv, "--coverage-weight", word], o)
        assert open(bed).read() == _bedgraph64(c.runs64(), names), word
        assert open(tsv).read() == _summary64(c.summary64(), names, tb["lens"]), word
        assert c.n_runs > 10000 and open(bed).read() != open(bed0).read()
        assert open(qt, "rb").read() == open(q0, "rb").read()
        # the main output and the final report are the run's without the switch
        h1, s1 = _body(o, False)
        assert h0 == h1 and np.array_equal(s0, s1) and len(s0) > 100000, word
        out0, out1 = r0.stdout.decode().split("\n"), r.stdout.decode().split("\n")
        line = [l for l in out1 if l.startswith("[bramble] coverage")]
        assert len(line) == 1 and line[0].startswith("[bramble] coverage (weight %s): %d records of weight " % (word, int(c.summary64()["records"].sum()))), line
        assert len(out1) == len(out0) and _report(r) == _report(r0) and len(_report(r)) == 5, word
        for p in (o, bed, tsv):
            assert os.path.exists(p) and not os.path.exists(p + ".tmp-bramble"), word
        q.close()
        c.close()
    # beside --sort, effective lengths, bootstraps, genes and --coverage-primary: the same join, the API's tables again
    q = _quant(tb["n_tx"], tb["lens"], eff_len=1)
    c = lib.Coverage(tb["lens"])
    c.set_param("weight", 2)
    c.set_param("primary_only", 1)
    _fill_last([q, c], tb)
    q.finish()
    q.em()
    c.finish_em(q)
    o, bed, tsv, qt = paths("all")
    _run([in_bam, "--sort", "-G", gtf, "--quant", qt, "--quant-eff-length", "--quant-bootstraps", "3", "--quant-genes", str(tmp_path / "genes.tsv"),
          "--coverage", bed, "--coverage-summary", tsv, "--coverage-primary", "--coverage-weight", "em"], o)
    assert open(bed).read() == _bedgraph64(c.runs64(), names) and open(tsv).read() == _summary64(c.summary64(), names, tb["lens"])
    assert 1000 < c.n_runs and int(c.stats()["rows_skipped"]) > 0
    q.close()
    c.close()

"""--quant-bootstraps on the GPU: the resampled class counts, every replicate's EM and the summary of br_quant_bootstrap against the
tests' restatement of the definitions (test_quant_boot_cpu.py), exactly: the counts as integers, theta and the summary bit for bit
(the hand-built wide input under the rule of test_gpu_quant.py, whose wave sums the sequential restatement does not order alike);
that the result does not depend on how the replicates are cut into chunks; what the call leaves alone and what it refuses; and the
command line."""
import functools
import math
import os

import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests.test_collate_cpu import collate_order, mapped_records
from tests.test_gpu_collate import _coordinate_stream, _files, _inputs, _report, _run
from tests.test_gpu_quant import _assert_em_to, _body, _fill, _hand_built, _new, _rows_a, _spread, _tables
from tests.test_quant_boot_cpu import boot_counts, boot_em, boot_summary
from tests.test_quant_cpu import classes_of, oracle_tables

pytestmark = pytest.mark.gpu

B = 6
NORM = {"pe": 1, "ont": 0}   # (the presets' defaults: test_gpu_quant.py's EM cases)


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same_bits(x, y):
    return np.array_equal(_bits(x), _bits(y))


@functools.lru_cache(maxsize=None)
def _classes(mode):
    tb = _tables(mode)
    return classes_of(tb["tids"], tb["row_off"], tb["group_off"])


@functools.lru_cache(maxsize=None)
def _ref_counts(mode, seed, n_boot=B):
    return np.asarray([boot_counts(_classes(mode)["counts"], seed, b) for b in range(n_boot)], dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def _ref_em(mode, seed, capped):
    """the restatement's (theta [B, T], n_iters [B]) of the B replicates at the preset's normalisation"""
    tb, kw = _tables(mode), ({"max_iters": 200, "tolerance": 0} if capped else {})
    runs = [boot_em(_classes(mode), tb["n_tx"], n, tb["lens"], bool(NORM[mode]), **kw) for n in _ref_counts(mode, seed)]
    return np.asarray([r["theta"] for r in runs]), [r["n_iters"] for r in runs]


def _boot(tb, how="host", length_norm=None, **params):
    q = _new(tb, length_norm=length_norm, **params)
    _fill(q, tb, how)
    q.finish()
    return q


def _simple(names):
    """every read name one alignment whose rows are the name's transcripts"""
    tids = np.asarray([t for nm in names for t in nm], dtype=np.uint32)
    row_off = np.concatenate([[0], np.cumsum([len(nm) for nm in names])]).astype(np.uint64)
    return tids, row_off, np.arange(len(names) + 1, dtype=np.uint32)


def _quant_of(names, n_tx, **params):
    tids, row_off, group_off = _simple(names)
    q = lib.Quant(n_tx)
    for k, v in params.items():
        q.set_param(k, v)
    q.add_host(_rows_a(tids), row_off, group_off)
    q.finish()
    return q


# ---- the resampled counts ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("seed", [0, (1 << 63) + 5])
def test_counts_match_the_restatement(mode, seed):
    tb = _tables(mode)
    q = _boot(tb, bootstraps=B, boot_seed=seed)
    assert q.classes()[2].tolist() == _classes(mode)["counts"]
    got = q.boot_counts()
    want = _ref_counts(mode, seed)
    assert got.shape == want.shape and got.dtype == np.uint32
    assert np.array_equal(got, want)
    assert np.array_equal(q.boot_counts(2, 3), want[2:5]) and np.array_equal(q.boot_counts(5, 1), want[5:])
    q.bootstrap()
    assert np.array_equal(q.boot_counts(1, 4), want[1:5])   # generated again, after the replicates ran as well
    q.close()


def _hand_tables():
    rng = np.random.RandomState(8)
    among = [[int(t)] for t in rng.permutation(np.repeat(np.arange(1, 51), 3))]
    bulk = [[0]] * 100000
    return {
        "one class": ([[5]] * 9, 8, 5),
        "70 000 classes of one name": ([[t] for t in range(70000)], 70000, 3),
        "100 000 names in one class among 50 others": (among[:70] + bulk + among[70:], 51, 3),
        "65 replicates": ([[int(t)] for t in rng.randint(0, 10, size=400)] + [[t] for t in range(10)], 10, 65),
        "no names with labels": ([[], [], []], 4, 3),
    }


@pytest.mark.parametrize("case", ["one class", "70 000 classes of one name", "100 000 names in one class among 50 others", "65 replicates",
                                  "no names with labels"])
def test_counts_on_hand_built_tables(case):
    names, n_tx, n_boot = _hand_tables()[case]
    q = _quant_of(names, n_tx, bootstraps=n_boot, boot_seed=12345)
    counts = q.classes()[2]
    cl = classes_of(*_simple(names))
    assert counts.tolist() == cl["counts"]
    if case == "100 000 names in one class among 50 others":
        assert len(counts) == 51 and int(counts.max()) == 100000
    if case == "65 replicates":
        assert len(counts) == 10
    got = q.boot_counts()
    want = np.asarray([boot_counts(counts, 12345, b) for b in range(n_boot)], dtype=np.uint32).reshape(n_boot, len(counts))
    assert np.array_equal(got, want)
    assert all(int(r.sum()) == int(counts.sum()) for r in got)
    if case == "no names with labels":
        assert q.n_classes == 0
        it = q.bootstrap()
        assert len(it) == 3 and not q.boot_theta().any()
        mean, var = q.boot_summary()
        assert not mean.any() and not var.any()
    q.close()


# ---- the replicates' EM -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("capped", [False, True])
def test_em_bits_match_the_restatement(mode, capped):
    tb = _tables(mode)
    want, want_iters = _ref_em(mode, 7, capped)
    print("%s: the restatement's replicates stop after %s iterations" % (mode, want_iters))
    params = {"max_iters": 200, "tolerance": 0} if capped else {}
    q = _boot(tb, length_norm=NORM[mode], bootstraps=B, boot_seed=7, **params)
    it = q.bootstrap()
    got = q.boot_theta()
    assert it.tolist() == want_iters
    if capped:
        assert want_iters == [200] * B
    else:
        assert len(set(want_iters)) > 1   # replicates of one chunk stop at different looks: the earlier ones stay frozen
    for b in range(B):
        assert _same_bits(got[b], want[b]), b
    assert _same_bits(q.boot_theta(2, 3), want[2:5])
    st = q.boot_stats()
    assert st["iterations_total"] == sum(want_iters) and st["sample_s"] > 0 and st["em_s"] > 0
    q.close()


def test_em_on_hand_built_wide_inputs():
    """a class of 200 labels and a transcript in 5 000 classes: a wave's sums, which the sequential restatement orders otherwise --
    within 64 s of it, s the restatement's own spread over three class orders (the rule of test_gpu_quant.py for this input)"""
    tids, row_off, group_off, n_tx = _hand_built()
    cl = classes_of(tids, row_off, group_off)
    q = lib.Quant(n_tx)
    for k, v in (("max_iters", 100), ("tolerance", 0), ("bootstraps", 3), ("boot_seed", 4)):
        q.set_param(k, v)
    q.add_host(_rows_a(tids), row_off, group_off)
    q.finish()
    assert q.bootstrap().tolist() == [100, 100, 100]
    got = q.boot_theta()
    counts = q.boot_counts()
    for b in range(3):
        assert np.array_equal(counts[b], boot_counts(cl["counts"], 4, b))
        ref, s = _spread(dict(cl, counts=[int(v) for v in counts[b]]), n_tx, None, False, 100)
        tot = 0.0
        for v in got[b]:   # TPM as br_quant_result makes it (w = 1), for the rule's second key
            tot += float(v)
        _assert_em_to({"theta": got[b], "tpm": 1e6 * got[b] / tot}, ref, s, 100, "hand-built, replicate %d" % b)
    q.close()
    # the same replicates as the first three of six, and of seventeen in chunks of sixteen (a wave carries a wide chunk through a
    # large item four replicates at a time, a chunk's frozen and unused columns beside them): the same bits
    for n_boot in (6, 17):
        q = lib.Quant(n_tx)
        for k, v in (("max_iters", 100), ("tolerance", 0), ("bootstraps", n_boot), ("boot_seed", 4)):
            q.set_param(k, v)
        q.add_host(_rows_a(tids), row_off, group_off)
        q.finish()
        assert q.bootstrap().tolist() == [100] * n_boot
        assert _same_bits(q.boot_theta(0, 3), got), n_boot
        if n_boot == 17:
            one = q.boot_theta(16, 1)
        q.close()
    q = lib.Quant(n_tx)
    for k, v in (("max_iters", 100), ("tolerance", 0), ("bootstraps", 17), ("boot_seed", 4), ("boot_chunk", 1)):
        q.set_param(k, v)
    q.add_host(_rows_a(tids), row_off, group_off)
    q.finish()
    q.bootstrap()
    assert _same_bits(q.boot_theta(16, 1), one) and _same_bits(q.boot_theta(0, 3), got)
    q.close()
    # to the default tolerance the replicates stop at looks of their own: a wave's items freeze as a lane's do
    runs = []
    for chunk in (1, 0):
        q = lib.Quant(n_tx)
        for k, v in (("max_iters", 2000), ("bootstraps", 5), ("boot_seed", 4), ("boot_chunk", chunk)):
            q.set_param(k, v)
        q.add_host(_rows_a(tids), row_off, group_off)
        q.finish()
        runs.append((q.bootstrap().tolist(), q.boot_theta()))
        q.close()
    print("hand-built: the replicates stop after %s iterations" % runs[0][0])
    assert runs[0][0] == runs[1][0] and _same_bits(runs[0][1], runs[1][1])


# ---- the result does not depend on the cut --------------------------------------------------------------------------------------------
def test_chunks_runs_and_adds_give_the_same_bits():
    tb = _tables("pe")
    want, want_iters = _ref_em("pe", 7, False)
    for how, chunk in (("host", 1), ("host", 4), ("host", 3), ("dev1", 0), ("dev3", 0), ("dev1", 0)):
        q = _boot(tb, how=how, length_norm=1, bootstraps=B, boot_seed=7, boot_chunk=chunk)
        it = q.bootstrap()
        assert it.tolist() == want_iters, (how, chunk)
        assert _same_bits(q.boot_theta(), want), (how, chunk)
        q.close()


def test_effective_lengths():
    from tests.test_gpu_quant_fld import _fill_rows, _tables as _fld_tables
    from tests.test_quant_fld_cpu import eff_lengths
    tb, _, pk, hist = _fld_tables("pe")
    eff = eff_lengths(hist["hist"], tb["lens"], 1000)
    cl = _classes("pe")
    q = _new(tb, eff_len=1, bootstraps=2, boot_seed=7)
    _fill_rows(q, pk, tb["row_off"], tb["group_off"], "dev1")
    q.finish()
    it = q.bootstrap()
    got = q.boot_theta()
    for b in range(2):
        ref = boot_em(cl, tb["n_tx"], _ref_counts("pe", 7)[b], eff, True)
        assert int(it[b]) == ref["n_iters"] and _same_bits(got[b], ref["theta"]), b
    assert not _same_bits(got[0], _ref_em("pe", 7, False)[0][0])   # (the effective lengths were used)
    q.close()


# ---- the summary ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_boot", [1, B])
def test_summary_bits(n_boot):
    tb = _tables("pe")
    q = _boot(tb, length_norm=1, bootstraps=n_boot, boot_seed=7, max_iters=200, tolerance=0)
    q.bootstrap()
    theta = q.boot_theta()
    assert _same_bits(theta, _ref_em("pe", 7, True)[0][:n_boot])
    mean, var = q.boot_summary()
    want_mean, want_var = boot_summary(theta)
    assert _same_bits(mean, want_mean) and _same_bits(var, want_var)
    assert (var > 0).any() == (n_boot > 1)
    q.close()


# ---- what the call leaves alone, and what it refuses ------------------------------------------------------------------------------
@pytest.mark.parametrize("first", ["em", "bootstrap"])
def test_point_result_is_untouched(first):
    tb = _tables("ont")
    plain = _boot(tb, length_norm=0, max_iters=200, tolerance=0)
    plain.em()
    want = plain.result()
    plain.close()
    q = _boot(tb, length_norm=0, max_iters=200, tolerance=0, bootstraps=3, boot_seed=1)
    if first == "em":
        q.em()
        before = q.result()
        q.bootstrap()
    else:
        q.bootstrap()
        q.em()
        before = q.result()
    after = q.result()
    for key in ("theta", "tpm"):
        assert _same_bits(before[key], want[key]) and _same_bits(after[key], want[key]), key
    for key in ("unique", "ambig"):
        assert np.array_equal(after[key], want[key])
    assert _same_bits(q.boot_theta(), _ref_em("ont", 1, True)[0][:3])
    st = q.stats()
    assert st["peak_bytes"] >= st["held_bytes"] >= 3 * tb["n_tx"] * 8
    q.close()


def test_refusals():
    L = lib.lib()
    tb = _tables("ont")
    out = np.zeros(B * max(tb["n_tx"], 4096), dtype=np.float64)
    q = _new(tb, bootstraps=2)
    assert L.br_quant_bootstrap(q.h, None) == -1                          # before finish
    assert L.br_quant_boot_counts(q.h, 0, 1, out.ctypes.data) == -1
    _fill(q, tb, "host")
    q.finish()
    assert L.br_quant_boot_theta(q.h, 0, 1, out.ctypes.data) == -1        # before bootstrap
    assert L.br_quant_boot_summary(q.h, out.ctypes.data, None) == -1
    for name, value in (("bootstraps", -1), ("bootstraps", 10001), ("boot_chunk", 65), ("boot_chunk", -1)):
        assert L.br_quant_set_param(q.h, name.encode(), value) == -1, name
    assert L.br_quant_set_param(q.h, b"max_iters", 5) == -1               # (the others stay closed after finish)
    q.set_param("bootstraps", 0)                                          # the three are open after finish
    assert L.br_quant_bootstrap(q.h, None) == -1                          # no replicates asked for
    assert L.br_quant_boot_counts(q.h, 0, 0, None) == -1
    q.set_param("bootstraps", 3)
    q.set_param("boot_seed", -2)
    q.set_param("boot_chunk", 64)
    for first, count in ((-1, 1), (0, -1), (3, 1), (2, 2)):
        assert L.br_quant_boot_counts(q.h, first, count, out.ctypes.data) == -1, (first, count)
    assert len(q.bootstrap()) == 3
    for first, count in ((-1, 1), (0, -1), (3, 1), (2, 2)):
        assert L.br_quant_boot_theta(q.h, first, count, out.ctypes.data) == -1, (first, count)
    for name in ("bootstraps", "boot_seed", "boot_chunk"):
        assert L.br_quant_set_param(q.h, name.encode(), 1) == -1, name     # closed once the replicates have run
    assert np.array_equal(q.boot_counts(0, 1)[0], boot_counts(_classes("ont")["counts"], -2, 0))
    q.close()
    q = lib.Quant(tb["n_tx"], tb["lens"])                                 # effective lengths without length normalisation: as br_quant_em
    q.set_param("eff_len", 1)
    q.set_param("length_norm", 0)
    q.set_param("bootstraps", 2)
    q.finish()
    assert L.br_quant_em(q.h, None, None) == -1 and L.br_quant_bootstrap(q.h, None) == -1
    q.close()


# ---- the command line -------------------------------------------------------------------------------------------------------------------
def _api_boot(tb, n_boot, seed):
    q = _new(tb, length_norm=1, bootstraps=n_boot, boot_seed=seed)
    q.add_host(_rows_a(tb["tids"]), tb["row_off"], tb["group_off"])
    q.finish()
    q.em()
    it = q.bootstrap()
    theta = q.boot_theta()
    mean, var = q.boot_summary()
    q.close()
    return theta, mean, var, int(it.sum())


def test_cli_bootstraps(tmp_path):
    annd, recs, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, hdr = _files(tmp_path, annd, stream, "in")
    sorted_bam, _ = _files(tmp_path, annd, _coordinate_stream(stream), "sorted")
    permuted = mapped_records(_coordinate_stream(stream))
    tb_in = oracle_tables("pe", guide_order=True)   # (the command line numbers the transcripts in guide order)
    tb_col = oracle_tables("pe", [permuted[i] for i in collate_order(permuted)], guide_order=True)
    tx_names = [t["id"] for t in tb_in["annd"]["transcripts"]]
    n_boot, seed = 4, 9
    runs = {"plain": ([in_bam], tb_in), "collate": ([sorted_bam, "--collate"], tb_col), "sort": ([in_bam, "--sort"], tb_in),
            "samout": ([in_bam, "-O", "sam"], tb_in)}
    api = {}
    for tag, (args, tb) in runs.items():
        if id(tb) not in api:
            api[id(tb)] = _api_boot(tb, n_boot, seed)
        theta, mean, var, iters = api[id(tb)]
        sam = tag == "samout"
        o0, o1 = str(tmp_path / ("quant_%s.out" % tag)), str(tmp_path / ("boot_%s.out" % tag))
        t0, t1, bo = str(tmp_path / ("%s.tsv" % tag)), str(tmp_path / ("%s.boot.tsv" % tag)), str(tmp_path / ("%s.reps.tsv" % tag))
        r0 = _run(args + ["-G", gtf, "--quant", t0], o0)
        r1 = _run(args + ["-G", gtf, "--quant", t1, "--quant-bootstraps", str(n_boot), "--quant-seed", str(seed), "--quant-boot-out", bo], o1)
        # the main output and the table's old columns: the bytes of the run without the switches
        if sam:
            assert _body(o0, True) == _body(o1, True)
        else:
            h0, s0 = _body(o0, False)
            h1, s1 = _body(o1, False)
            assert h0 == h1 and np.array_equal(s0, s1) and len(s0) > 100000, tag
        lines = open(t1).read().split("\n")
        assert lines[-1] == "" and lines[0].split("\t")[-2:] == ["BootMean", "BootSD"], tag
        assert "\n".join("\t".join(l.split("\t")[:-2]) for l in lines[:-1]) + "\n" == open(t0).read(), tag
        # the new columns and the replicates' file: the API's values, printed alike
        assert [l.split("\t")[-2:] for l in lines[1:-1]] == [["%.6f" % m, "%.6f" % math.sqrt(v)] for m, v in zip(mean, var)], tag
        reps = open(bo).read().split("\n")
        assert reps[-1] == "" and reps[0] == "\t".join(["Name"] + [str(b) for b in range(n_boot)]), tag
        assert reps[1:-1] == ["\t".join([nm] + ["%.6f" % theta[b][t] for b in range(n_boot)]) for t, nm in enumerate(tx_names)], tag
        # the report
        out0, out1 = r0.stdout.decode().split("\n"), r1.stdout.decode().split("\n")
        line = "[bramble] bootstrapped %d replicates (seed %d, %d iterations in all, sampling " % (n_boot, seed, iters)
        at = [k for k, l in enumerate(out1) if l.startswith(line)]
        assert len(at) == 1 and out1[at[0] + 1].startswith("[bramble] quantified "), (tag, [l for l in out1 if "bootstrapped" in l])
        assert not any("bootstrapped" in l for l in out0)
        assert _report(r1) == _report(r0)
        for p in (t1, bo, o1):
            assert os.path.exists(p) and not os.path.exists(p + ".tmp-bramble")

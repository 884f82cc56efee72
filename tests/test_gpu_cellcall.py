"""br_cellcall on the GPU against its restatement (tests/cellcall_cases.py).  The restatement is fed the object's own p, lp, ln and T
tables, so everything behind them -- ranks, thresholds, ambient counts, log-likelihoods, every simulation, p-values, the called
set -- is compared bit for bit; the tables themselves are compared with numpy."""
import numpy as np
import pytest

from bramble_amd import lib
from tests import cellcall_cases as cc

pytestmark = pytest.mark.gpu

INVALID = -1
_OBJECT = ("method", "expected", "ind_min", "ind_max", "umi_min", "cand_max", "sims", "seed", "percentile", "ratio", "umi_frac", "fdr")


def _run(off, feat, cnt, F, P, **extra):
    c = lib.CellCall(**{k: P[k] for k in _OBJECT}, **extra)
    return c.run(off, feat, cnt, F)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(off, feat, cnt, F, P, **extra):
    """One run compared with the restatement in full -> (the object, its stats, the restatement's result)"""
    return _compare(_run(off, feat, cnt, F, P, keep_sims=1, **extra), off, feat, cnt, F, P)


def _compare(c, off, feat, cnt, F, P):
    st = c.stats()
    given = None
    if P["method"] == 2 and st["fallback"] in (0, 3) and st["window"]:
        a = c.ambient()
        given = dict(p=a["p"], lp=a["lp"], T=a["T"])
        if st["candidates"]:
            given["ln"] = c.logtable()
    R = cc.call(off, feat, cnt, F, P, given=given, keep_sims=True)
    status, rank, total = c.calls()
    assert np.array_equal(total, R["total"]) and np.array_equal(rank, R["rank"])
    assert st["threshold"] == R["threshold"] and st["n_simple"] == R["n_simple"] and st["fallback"] == R["fallback"]
    assert st["candidates"] == R["candidates"]
    assert np.array_equal(status, R["status"])
    assert st["called_simple"] == int(np.sum(R["status"] == 1))
    assert st["called_emptydrops"] == int(np.sum(R["status"] == 2))
    if "amb" in R:
        assert np.array_equal(c.ambient(counts_only=True)["amb"], R["amb"]) and st["ambient_counts"] == int(R["amb"].sum())
        assert st["active_features"] == int(R["active"].sum()) and st["window"] == R["window"]
    if R["candidates"]:
        k = c.candidates()
        assert np.array_equal(k["cell"], R["cand"]) and st["n_max"] == R["n_max"] and st["lo"] == R["lo"]
        assert np.array_equal(c.wanted(), R["wanted"])
        assert np.array_equal(_bits(k["O"]), _bits(R["O"]))
        assert np.array_equal(_bits(c.sims()), _bits(R["L"]))
        assert np.array_equal(k["lower"], R["lower"])
        assert np.array_equal(_bits(k["pval"]), _bits(R["pval"])) and np.array_equal(_bits(k["padj"]), _bits(R["padj"]))
    return c, st, R


def _within_ulps(got, want, n):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    return np.array_equal(got[~fin], want[~fin]) and bool(np.all(np.abs(got[fin] - want[fin]) <= n * np.spacing(np.abs(want[fin]))))


def _planted(seed):
    d, planted, ambient_like, P = cc.planted(seed)
    return cc.csr(d) + (d.shape[1], P, planted, ambient_like)


def test_tables():
    off, feat, cnt, F, P, _, _ = _planted(1)
    c = _run(off, feat, cnt, F, P)
    a, ln, st = c.ambient(), c.logtable(), c.stats()
    active = np.zeros(F, np.uint8)
    active[feat] = 1
    ref_p, info = cc.sgt(a["amb"], active)
    assert st["p_route"] == info["route"] and _within_ulps([st["slope"]], [info["slope"]], 64)
    assert np.allclose(a["p"], ref_p, rtol=2.0 ** -40, atol=0)      # (test_cellcall_cpu.py holds the host routine to its bound)
    with np.errstate(divide="ignore"):
        assert _within_ulps(a["lp"][active == 1], np.log(a["p"][active == 1]), 2) and np.all(a["lp"][active == 0] == 0)
    assert len(ln) == st["n_max"] + 2 and ln[0] == 0 and _within_ulps(ln[1:], np.log(np.arange(1, len(ln), dtype=np.float64)), 2)
    assert np.array_equal(a["T"], cc.thresholds(a["p"], active))


_TOTALS = {"ties": [5, 9, 7, 7, 0, 7, 2], "cr": [100, 96, 50, 10, 10, 9, 1, 10], "one": [4], "none": [], "zeros": [0, 0],
           "many": list(np.random.default_rng(3).integers(0, 3000, 5000))}


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("shape", sorted(_TOTALS))
def test_ranks_thresholds_and_statuses(method, shape):
    off, feat, cnt = cc.csr(cc.dense_of_totals(_TOTALS[shape]))
    for kw in (dict(expected=3), dict(expected=200, ratio=5.0), dict(expected=3000)):
        P = dict(cc.DEFAULTS, method=method, sims=8, **kw)    # (method 2: the default window is empty: the simple result)
        _, st, R = _check(off, feat, cnt, 3, P)
        assert st["cells"] == len(_TOTALS[shape]) and st["fallback"] == (1 if method == 2 and len(_TOTALS[shape]) else 0)


def _tied_matrix():
    rng = np.random.default_rng(8)
    totals = [900, 40, 30] + [5] * 9 + [1, 1, 0, 0, 0]
    return cc.csr(np.stack([rng.multinomial(t, np.full(12, 1.0 / 12)) for t in totals]))


def test_ambient_window_through_a_run_of_ties():
    off, feat, cnt = _tied_matrix()
    P = dict(cc.DEFAULTS, expected=1, ind_min=5, ind_max=9, umi_min=1, umi_frac=0.0, sims=33, seed=3)
    _, st, R = _check(off, feat, cnt, 12, P)
    assert st["window"] == 4 and st["ambient_counts"] == 20 and st["fallback"] == 0 and st["candidates"] == 13


def test_empty_and_zero_sum_windows():
    off, feat, cnt = _tied_matrix()
    for window, word in (((40, 90), 1), ((9, 9), 1), ((14, 17), 2)):
        P = dict(cc.DEFAULTS, expected=1, ind_min=window[0], ind_max=window[1], umi_min=1, sims=9)
        c, st, R = _check(off, feat, cnt, 12, P)
        assert st["fallback"] == word and st["called_emptydrops"] == 0
        simple = _run(off, feat, cnt, 12, dict(P, method=1)).calls()
        assert all(np.array_equal(x, y) for x, y in zip(c.calls(), simple))


@pytest.mark.parametrize("n_active,n_max,sims,heavy", [(1, 1, 1, False), (2, 63, 63, False), (65, 64, 65, False), (1000, 65, 300, False),
                                                       (2, 257, 65, False), (65, 257, 300, False), (1000, 257, 63, False), (1, 64, 300, False),
                                                       (65, 1, 65, False), (1000, 63, 1, False), (2, 65, 300, True), (65, 257, 65, True)])
def test_simulations(n_active, n_max, sims, heavy):
    off, feat, cnt, F, P = cc.sim_case(n_active, n_max, heavy=heavy, seed=n_active + sims, K_tail=4000 if heavy else 40)
    P = dict(P, sims=sims)
    c, st, R = _check(off, feat, cnt, F, P)
    assert st["active_features"] == n_active and st["n_max"] == n_max and st["fallback"] == 0 and st["sim_chunks"] == 1
    if heavy:   # one feature holds 0.95 of the mass or more: most lanes of a step draw it
        assert c.ambient()["p"].max() >= 0.95


def test_chunked_simulations_are_the_same():
    off, feat, cnt, F, P = cc.sim_case(65, 257, seed=2)
    P = dict(P, sims=300)
    one, st1, _ = _check(off, feat, cnt, F, P)
    cut, st3, _ = _check(off, feat, cnt, F, P, sim_bytes=65 * 4 * 100)
    tiny = _run(off, feat, cnt, F, P, keep_sims=1, sim_bytes=0)      # (one simulation a launch)
    assert st1["sim_chunks"] == 1 and st3["sim_chunks"] == 3 and tiny.stats()["sim_chunks"] == 300
    assert np.array_equal(_bits(one.sims()), _bits(cut.sims())) and np.array_equal(_bits(one.sims()), _bits(tiny.sims()))
    assert np.array_equal(_bits(one.sims(7, 5, 1, 2)), _bits(one.sims()[1:3, 7:12]))
    assert st3["peak_bytes"] < st1["peak_bytes"]
    dropped = _run(off, feat, cnt, F, P)
    assert dropped._raw("sims", 0, 1, 0, 1, None) == INVALID
    assert np.array_equal(dropped.candidates()["lower"], one.candidates()["lower"])


@pytest.mark.parametrize("seed", [1, 4])
def test_planted_matrix(seed):
    off, feat, cnt, F, P, planted, ambient_like = _planted(seed)
    c, st, R = _check(off, feat, cnt, F, P)
    assert st["candidates"] == 80 and st["called_simple"] == 30
    lower = c.candidates()["lower"]
    assert len(lower) - len(np.unique(lower)) >= 1          # two candidates of equal `lower`: the tie order of the adjustment
    # (test_cellcall_cpu.py: the restatement calls all the planted cells here, and at most 2 of the ambient-like ones)
    assert np.all(c.calls()[0][planted] == 2)


def test_fewer_candidates_than_there_are():
    off, feat, cnt, F, P, _, _ = _planted(1)
    c, st, R = _check(off, feat, cnt, F, dict(P, cand_max=50, sims=200))
    assert st["candidates"] == 50 and np.array_equal(c.candidates()["cell"], R["order"][30:80])


def test_device_tables():
    import torch
    off, feat, cnt, F, P, _, _ = _planted(4)
    P = dict(P, sims=100)
    host = _run(off, feat, cnt, F, P)
    dev = lib.CellCall(**{k: P[k] for k in _OBJECT})
    t = [torch.from_numpy(x.view(s)).cuda() for x, s in ((off, np.int64), (feat, np.int32), (cnt, np.int32))]
    dev.run_device(t[0], t[1], t[2], F)
    assert all(np.array_equal(x, y) for x, y in zip(host.calls(), dev.calls()))
    assert all(np.array_equal(_bits(host.candidates()[k]), _bits(dev.candidates()[k])) for k in ("O", "pval", "padj"))
    # the checks of a device matrix are the kernel's: offsets that descend, a feature out of range
    bad = off.copy()
    bad[2], bad[3] = off[3], off[2]
    for o, n_features in ((bad, F), (off, F - 1)):
        again = lib.CellCall(**{k: P[k] for k in _OBJECT})
        d_off = torch.from_numpy(o.view(np.int64)).cuda()
        assert again.run_raw(len(off) - 1, n_features, d_off.data_ptr(), t[1].data_ptr(), t[2].data_ptr(), True) == INVALID
        again.run_device(t[0], t[1], t[2], F)
        assert np.array_equal(again.calls()[0], host.calls()[0])


def test_refusals():
    off, feat, cnt = cc.csr([[3, 0, 2], [0, 1, 0], [4, 4, 4]])
    P = dict(cc.DEFAULTS, method=1)

    def raw(o, f, k, F=3, n=None):
        c = lib.CellCall(method=1)
        o, f, k = np.array(o, np.uint64), np.array(f, np.uint32), np.array(k, np.uint32)
        rc = c.run_raw(len(o) - 1 if n is None else n, F, o.ctypes.data, f.ctypes.data, k.ctypes.data)
        if rc:   # a refused run has changed nothing: the object takes parameters and runs
            c.set_param("expected", 2)
            c.run(off, feat, cnt, 3)
            assert list(c.calls()[2]) == [5, 1, 12]
        return rc

    assert raw(off, feat, cnt) == 0
    assert raw([0, 2, 1, 6], feat, cnt) == INVALID            # offsets that descend
    assert raw([1, 2, 3, 6], feat, cnt) == INVALID            # ... that do not start at 0
    assert raw(off, [0, 2, 3, 0, 1, 2], cnt) == INVALID       # a feature out of range
    assert raw(off, feat, cnt, F=2) == INVALID
    assert raw(off, [2, 0, 1, 0, 1, 2], cnt) == INVALID       # features not ascending
    assert raw(off, [0, 0, 1, 0, 1, 2], cnt) == INVALID
    assert raw(off, feat, [3, 2, 1, 4, 0, 4]) == INVALID      # a count of 0
    assert raw([0, 2], [0, 1], [0xffffffff, 1], F=2) == INVALID   # a total of 2^32
    assert raw([0, 2], [0, 1], [0xfffffffe, 1], F=2) == 0
    c = _run(off, feat, cnt, 3, P)
    assert c._raw("set_param", b"expected", 5) == INVALID and c._raw("set_real", b"ratio", 2.0) == INVALID   # after run
    assert c.run_raw(3, 3, off.ctypes.data, feat.ctypes.data, cnt.ctypes.data) == INVALID                    # a second run
    assert c._raw("ambient", 0, 3, None, None, None, None) == INVALID and c._raw("calls", 1, 3, None, None, None) == INVALID
    fresh = lib.CellCall()
    assert fresh._raw("calls", 0, 0, None, None, None) == INVALID                                            # before run
    for name, v in (("method", 3), ("expected", 0), ("sims", 0), ("cand_max", 0), ("keep_sims", 2), ("nothing", 1)):
        assert fresh._raw("set_param", name.encode(), v) == INVALID
    for name, v in (("percentile", 1.5), ("ratio", 0.5), ("fdr", -0.1), ("umi_frac", float("nan")), ("nothing", 1.0)):
        assert fresh._raw("set_real", name.encode(), v) == INVALID


# ---- through br_cells ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("mode", ["unique", "uniform", "em"])
def test_through_cells(mode, method):
    from tests import cells_cases as cells
    from tests import test_gpu_cells as tgc
    c, q = tgc._run("standard", "host", mode=lib.Cells.MODES[mode], call_counts=1)
    u = tgc._want("standard", "unique")                      # the cells are called on the unique counts whatever the mode
    off, feat, cnt = np.asarray(u["off"], np.uint64), np.asarray(u["feature"], np.uint32), np.asarray(u["value"]).astype(np.uint32)
    assert np.array_equal(cnt, np.asarray(u["value"])) and cnt.min() > 0
    K = c.n_cells
    P = dict(cc.DEFAULTS, method=method, expected=max(2, K // 8), ratio=3.0, ind_min=K // 2, ind_max=K, umi_min=1, umi_frac=0.0, sims=50, seed=9)
    call = c.call(lib.CellCall(**{k: P[k] for k in _OBJECT}, keep_sims=1), cells.N_FEATURES)
    _, st, R = _compare(call, off, feat, cnt, cells.N_FEATURES, P)
    assert st["cells"] == K and 0 < st["called_simple"] < K and (method != 2 or st["fallback"] == 0)
    # the called cells' rows of the mode's matrix, selected on the device
    moff, mfeat, mval = c.matrix()
    keep = np.nonzero(R["status"])[0]
    got_cells, goff, gfeat, gval = c.matrix_called()
    assert np.array_equal(got_cells, keep) and np.array_equal(np.diff(goff.astype(np.int64)), np.diff(moff.astype(np.int64))[keep])
    rows = np.concatenate([np.arange(moff[k], moff[k + 1], dtype=np.int64) for k in keep])
    assert np.array_equal(gfeat, mfeat[rows]) and np.array_equal(_bits(gval), _bits(mval[rows]))
    part = c.matrix_called(1, 2)
    assert np.array_equal(part[0], keep[1:3]) and np.array_equal(part[2], gfeat[goff[1]:goff[3]])
    assert c._raw("call", lib.CellCall().h, cells.N_FEATURES) == INVALID      # a second time


def test_cells_without_call_counts_refuse():
    from tests import cells_cases as cells
    from tests import test_gpu_cells as tgc
    c, q = tgc._run("standard", "host")
    plain = lib.CellCall(method=0)
    assert c._raw("call", plain.h, cells.N_FEATURES) == INVALID
    assert c._raw("matrix_called", 0, 0, None, np.zeros(1, np.uint64).ctypes.data, None, None) == INVALID
    c2, _ = tgc._run("standard", "host", finish=False, call_counts=1)
    assert c2._raw("call", plain.h, cells.N_FEATURES) == INVALID              # before finish
    assert plain._raw("set_param", b"expected", 5) == 0                        # (the caller is as it was)

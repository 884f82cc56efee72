"""The restatement of br_cellcall (tests/cellcall_cases.py) pinned by hand, the host-only br_cellcall_sgt against it, and the
conditions that tests/test_gpu_cellcall.py relies on for its inputs.  No GPU."""
import functools
import math

import numpy as np
import pytest

from bramble_amd import lib
from tests import cellcall_cases as cc


def _simple(totals, method, **kw):
    P = dict(cc.DEFAULTS, method=method, **kw)
    off, feat, cnt = cc.csr(cc.dense_of_totals(totals))
    return cc.call(off, feat, cnt, 3, P)


def test_topcells_by_hand():
    totals = [5, 9, 7, 7, 0, 7, 2]
    R = _simple(totals, 0, expected=3)
    assert list(R["order"]) == [1, 2, 3, 5, 0, 6, 4]          # ties by ascending cell index
    assert list(R["rank"]) == [4, 0, 1, 2, 6, 3, 5]
    assert R["threshold"] == 7 and R["n_simple"] == 4         # rank 2 holds 7; the tie at the threshold (cell 5) is in
    assert list(R["status"]) == [0, 1, 1, 1, 0, 1, 0]
    R = _simple(totals, 0, expected=100)                      # K < expected: the last rank's total is 0, the threshold max(0, 1)
    assert R["threshold"] == 1 and R["n_simple"] == 6 and R["status"][4] == 0
    R = _simple([4], 0, expected=3)                           # K = 1
    assert R["threshold"] == 4 and list(R["status"]) == [1]
    R = _simple([], 0, expected=3)
    assert R["n_simple"] == 0 and len(R["status"]) == 0


def test_cr22_by_hand():
    totals = [100, 96, 50, 10, 10, 9, 1, 10]
    # r = (int64)(200 * (1 - 0.99)) = 2 (200 * 0.010000000000000009 = 2.0000000000000018), tmax = 50, tmin = (int64)(50 / 5 + 0.5) = 10
    R = _simple(totals, 1, expected=200, percentile=0.99, ratio=5.0)
    assert R["threshold"] == 10 and R["n_simple"] == 6        # the three tens are all in
    assert list(R["status"]) == [1, 1, 1, 1, 1, 0, 0, 1]
    # r = min(K - 1, 30): K < expected takes the last rank, total 1: tmin = max(1, (int64)(0.1 + 0.5)) = 1
    R = _simple(totals, 1, expected=3000, percentile=0.99, ratio=10.0)
    assert R["threshold"] == 1 and R["n_simple"] == 8
    # rounding: tmax = 96 at r = 1, 96 / 10 + 0.5 = 10.1 -> 10; tmax = 100 at r = 0, ratio 8: 12.5 + 0.5 = 13
    assert _simple(totals, 1, expected=100, percentile=0.99, ratio=10.0)["threshold"] == 10
    assert _simple(totals, 1, expected=1, percentile=0.99, ratio=8.0)["threshold"] == 13
    R = _simple([7], 1)                                      # K = 1
    assert R["threshold"] == 1 and list(R["status"]) == [1]
    R = _simple([0, 0], 1)                                   # nothing has a count: tmin = 1, nobody called
    assert R["threshold"] == 1 and R["n_simple"] == 0


def test_sgt_by_hand():
    # active counts 1 1 1 1 2 2 4 0 0 and one inactive feature: n_1 = 4, n_2 = 2, n_4 = 1, n_0 = 2, N = 12.  r = 1, 2, 4, r_0 = 0,
    # r_4 = 6: Z = 8 / 2, 4 / 3, 2 / 4; log Z against log r is the line through (0, 2 ln 2), (2 ln 2, -ln 2) up to the middle
    # point, whose dx is 0: b = ln 2 (-3 ln 2) / (2 ln^2 2) = -1.5.  y(r) = r (1 + 1 / r)^-0.5.  At r = 1: x = 2 * 2 / 4 = 1, sd =
    # sqrt(4 * (2 / 16) * 1.5) = 0.866, |1 - 0.7071| <= 1.96 sd: switched at once, r* = y(r) throughout
    amb = [1, 0, 1, 2, 0, 1, 4, 2, 0, 1]
    active = [1, 1, 1, 1, 0, 1, 1, 1, 1, 1]
    p, info = cc.sgt(amb, active)
    assert info["route"] == 0 and info["distinct"] == 3 and abs(info["slope"] + 1.5) < 1e-14
    y = {r: r * (1.0 + 1.0 / r) ** -0.5 for r in (1, 2, 4)}
    Np = 4 * y[1] + 2 * y[2] + y[4]
    want = [(2.0 / 3.0) * y[a] / Np if a else 1.0 / 6.0 for a in amb]
    want[4] = 0.0
    assert np.allclose(p, want, rtol=1e-13, atol=0) and abs(p.sum() - 1.0) < 1e-5
    assert abs(p[0] - 0.048738) < 1e-6 and abs(p[6] - 0.246599) < 1e-6
    # no active feature with count 0: P0 = 0
    p2, _ = cc.sgt([1, 1, 1, 1, 2, 2, 4], [1] * 7)
    assert np.allclose(p2, [y[a] / Np for a in (1, 1, 1, 1, 2, 2, 4)], rtol=1e-13)


def test_sgt_add_one():
    p, info = cc.sgt([3, 3, 0, 0], [1, 1, 1, 0])             # m < 2
    assert info["route"] == 1 and list(p) == [4.0 / 9.0, 4.0 / 9.0, 1.0 / 9.0, 0.0]
    p, info = cc.sgt([1, 2, 3], [1, 1, 1])                    # Z = 1, 1, 1: slope 0, not below -1
    assert info["route"] == 1 and info["slope"] == 0.0 and list(p) == [2.0 / 9.0, 3.0 / 9.0, 4.0 / 9.0]


def test_bh_by_hand():
    # sims = 9: pval = 1, .1, .5, .1, 1; sorted by (lower, rank): places 1 .. 5 = candidates 1, 3, 2, 0, 4; q = .5, .25, .8333, 1.25 -> 1, 1
    pval, padj, called = cc.bh([9, 0, 4, 0, 9], 9, 0.3)
    assert list(pval) == [1.0, 0.1, 0.5, 0.1, 1.0]
    assert list(padj) == [1.0, 0.25, 0.5 * 5.0 / 3.0, 0.25, 1.0]
    assert list(called) == [False, True, False, True, False]
    # the tie's order: the earlier rank takes the earlier place, so its q is the larger one and its padj the running minimum
    pval, padj, _ = cc.bh([2, 2], 9, 0.5)
    assert list(padj) == [0.3, 0.3]


def test_threshold_table():
    rng = np.random.default_rng(5)
    F = 40
    active = (np.arange(F) % 3 != 1).astype(np.uint8)
    active[-4:] = 0
    active[0] = 0
    p = np.where(active, rng.gamma(0.3, 1.0, F) + 1e-7, 0.0)
    p /= p.sum()
    T = cc.thresholds(p, active)
    last = int(np.nonzero(active)[0][-1])
    assert np.all(np.diff(T.astype(np.int64)) >= 0) and int(T[last]) == 1 << 32 and np.all(T[last:] == 1 << 32) and T[0] == 0
    g = cc.pick(T, np.arange(1 << 16, dtype=np.uint64) << np.uint64(16))
    assert g.max() <= last and np.all(active[g] == 1)
    assert int(cc.pick(T, np.array([0xffffffff], np.uint64))[0]) <= last
    # the picks' frequencies are the probabilities up to the table's grain
    freq = np.bincount(g, minlength=F) / float(1 << 16)
    assert np.abs(freq - p).max() < 2.0 / (1 << 16)


def _ambient_vectors():
    rng = np.random.default_rng(11)
    out = []
    for i in range(20):
        F = int(rng.integers(30, 400))
        active = (rng.random(F) < 0.8).astype(np.uint8)
        prof = rng.gamma(0.2 + 0.1 * (i % 5), 1.0, F) * active
        amb = rng.multinomial(int(rng.integers(50, 20000)), prof / prof.sum()) if i < 18 else np.where(active, 3 if i == 18 else np.arange(F) % 3 + 1, 0)
        out.append((amb.astype(np.uint64), active))
    return out


def test_library_sgt_against_the_restatement():
    worst, spread, routes = 0.0, 0.0, set()
    for amb, active in _ambient_vectors():
        got, info = lib.CellCall.sgt(amb, active)
        ref, rinfo = cc.sgt(amb, active)
        assert info["route"] == rinfo["route"] and info["distinct"] == rinfo["distinct"] and info["active"] == int(active.sum())
        assert np.all((got > 0) == (ref > 0)) and np.all(got[active == 0] == 0)
        routes.add(info["route"])
        nz = ref > 0
        for variant in (dict(order="reversed"), dict(order="shuffle", shuffle_seed=7), dict(log=np.log)):
            v, _ = cc.sgt(amb, active, **variant)
            spread = max(spread, float(np.max(np.abs(v[nz] - ref[nz]) / ref[nz])))
        worst = max(worst, float(np.max(np.abs(got[nz] - ref[nz]) / ref[nz])))
    assert routes == {0, 1}
    bound = max(64.0 * spread, 2.0 ** -44)
    print("br_cellcall_sgt: largest relative difference %.3g, variants' spread %.3g, bound %.3g" % (worst, spread, bound))
    # observed: largest relative difference 0 (the host routine and the restatement share one libm), spread 7.1e-16, bound 5.7e-14 (the floor, 2^-44)
    assert worst <= bound


@functools.lru_cache(maxsize=None)
def planted_result(seed):
    d, planted, ambient_like, P = cc.planted(seed)
    off, feat, cnt = cc.csr(d)
    return cc.call(off, feat, cnt, d.shape[1], P), planted, ambient_like


@pytest.mark.parametrize("seed", [1, 4])
def test_planted_cells_are_called(seed):
    """400 barcodes x 120 features: 30 large cells, 40 small cells of a profile unlike the ambient one, 40 barcodes of the same
    totals from the ambient profile, and the ambient tail (the window).  Seed 1 takes the Good-Turing route, seed 4 add-one."""
    R, planted, ambient_like = planted_result(seed)
    assert R["fallback"] == 0 and R["n_simple"] == 30 and R["candidates"] == 80 and R["sgt"]["route"] == (0 if seed == 1 else 1)
    assert np.all(R["status"][planted] == 2)
    assert int(np.sum(R["status"][ambient_like] == 2)) <= 2
    assert int(np.sum(R["status"] == 1)) == 30

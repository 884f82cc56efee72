"""br_cellcall restated in plain Python / numpy float64, step by step as include/bramble_amd.h defines it, and the builders of
the matrices the cell calling tests use.  Nothing here loads the library."""
import math

import numpy as np

from tests.test_quant_boot_cpu import philox4x32_10

DEFAULTS = dict(method=2, expected=3000, percentile=0.99, ratio=10.0, ind_min=45000, ind_max=90000, umi_min=500, umi_frac=0.01,
                cand_max=20000, fdr=0.01, sims=10000, seed=0)
NONE = 0xffffffff


# ---- matrices ---------------------------------------------------------------------------------------------------------------
def csr(dense):
    """a dense K x F count array -> (cell_off uint64, feature uint32, count uint32)"""
    dense = np.asarray(dense, dtype=np.int64)
    off, feat, cnt = [0], [], []
    for row in dense:
        g = np.nonzero(row)[0]
        feat.extend(g.tolist()); cnt.extend(row[g].tolist()); off.append(len(feat))
    return np.array(off, np.uint64), np.array(feat, np.uint32), np.array(cnt, np.uint32)


def dense_of_totals(totals, n_features=3):
    """cells of the given totals: the total spread over the first features, one count at least where there is one"""
    K = len(totals)
    d = np.zeros((K, n_features), np.int64)
    for c, t in enumerate(totals):
        d[c, 0] = t - t // 2
        d[c, 1 % n_features] += t // 2
    return d


def draw_cells(rng, totals, profile):
    return np.stack([rng.multinomial(int(t), profile) for t in totals]) if len(totals) else np.zeros((0, len(profile)), np.int64)


def planted(seed, K=400, F=120, n_large=30, n_small=40):
    """-> (dense K x F, planted cell indices, ambient-like cell indices, params).  Large cells and n_small small ones drawn from
    a cell profile, n_small barcodes of the same totals and a tail drawn from the ambient profile; the rows shuffled."""
    rng = np.random.default_rng(seed)
    amb = rng.gamma(0.5, 1.0, F) + 0.02
    amb /= amb.sum()
    cell = rng.permutation(amb) * rng.gamma(2.0, 1.0, F)
    cell /= cell.sum()
    small_tot = rng.integers(60, 121, n_small)
    rows = [draw_cells(rng, rng.integers(2000, 4001, n_large), cell), draw_cells(rng, small_tot, cell), draw_cells(rng, small_tot, amb),
            draw_cells(rng, rng.integers(1, 16, K - n_large - 2 * n_small), amb)]
    d = np.concatenate(rows)
    perm = rng.permutation(K)
    out = np.zeros_like(d)
    out[perm] = d
    params = dict(DEFAULTS, expected=n_large, ind_min=n_large + 2 * n_small + 40, ind_max=K, umi_min=20, sims=1000, seed=12345)
    return out, np.sort(perm[n_large:n_large + n_small]), np.sort(perm[n_large + n_small:n_large + 2 * n_small]), params


def sim_case(n_active, n_max, n_inactive_every=3, heavy=False, seed=0, K_tail=40):
    """A matrix whose emptydrops run has `n_active` active features (an inactive one after every n_inactive_every-th), one simple
    cell and candidates whose largest total is n_max.  heavy: the ambient profile has 0.98 of its mass on one feature.
    -> (cell_off, feature, count, F, params)"""
    rng = np.random.default_rng(seed + 1000 * n_active + n_max)
    act = []
    g = 0
    while len(act) < n_active:
        if n_inactive_every and (g % (n_inactive_every + 1)) == n_inactive_every:
            g += 1
            continue
        act.append(g); g += 1
    F = g + 2   # (two trailing inactive features)
    act = np.array(act)
    prof = rng.gamma(0.7, 1.0, n_active) + 0.05
    if heavy:
        prof = prof / prof.sum() * 0.02
        prof[n_active // 2] = 0.98
    prof /= prof.sum()
    cell_prof = rng.permutation(prof)
    big = 50 * n_max + 1000
    totals_c = sorted({n_max, max(1, n_max // 2), max(1, n_max - 1), 1 if n_max < 4 else 3}, reverse=True)
    d = np.zeros((1 + len(totals_c) + K_tail, F), np.int64)
    d[0, act] = rng.multinomial(big, cell_prof) + 1   # (every one of them is active)
    for i, t in enumerate(totals_c):
        d[1 + i, act] = rng.multinomial(t, cell_prof if i % 2 == 0 else prof)
    for i in range(K_tail):
        d[1 + len(totals_c) + i, act] = rng.multinomial(1 + (i % 3 == 0 and n_max >= 3), prof)
    # (rank order = row order: the tail's totals are at most 2, below or equal to the smallest candidate's)
    off, feat, cnt = csr(d)
    n_c = 1 + len(totals_c)
    params = dict(DEFAULTS, expected=1, umi_min=1, umi_frac=0.0, ind_min=n_c, ind_max=d.shape[0], cand_max=len(totals_c), sims=64, seed=seed)
    return off, feat, cnt, F, params


# ---- the definitions --------------------------------------------------------------------------------------------------------
def totals_and_order(cell_off, count):
    off = np.asarray(cell_off, dtype=np.int64)
    c64 = np.asarray(count, dtype=np.int64)
    total = np.array([c64[off[c]:off[c + 1]].sum() for c in range(len(off) - 1)], dtype=np.int64)
    key = [((0xffffffff - int(t)) << 32) | c for c, t in enumerate(total)]
    order = np.array(sorted(range(len(key)), key=key.__getitem__), dtype=np.int64)
    rank = np.zeros(len(order), np.int64)
    rank[order] = np.arange(len(order))
    return total, order, rank


def simple_threshold(sorted_totals, method, expected, percentile, ratio):
    """sorted_totals: the totals in rank order -> (threshold, the length of the called rank prefix)"""
    K = len(sorted_totals)
    if K == 0:
        return 0, 0
    if method == 0:
        thr = max(int(sorted_totals[min(expected, K) - 1]), 1)
    else:
        r = min(K - 1, int(float(expected) * (1.0 - percentile)))
        tmax = int(sorted_totals[r])
        thr = max(1, int(float(tmax) / ratio + 0.5))
    return thr, int(np.sum(np.asarray(sorted_totals) >= thr))


def sgt(amb, active, log=math.log, order="forward", shuffle_seed=0):
    """-> (p float64 per feature, dict route / slope / distinct).  order: how the regression's sums run (the definition: forward)"""
    amb = [int(a) for a in amb]
    act = [g for g in range(len(amb)) if active[g]]
    N = sum(amb[g] for g in act)
    counts = sorted(amb[g] for g in act)
    n0 = sum(1 for x in counts if x == 0)
    rv = sorted({x for x in counts if x > 0})
    nr = [counts.count(x) for x in rv]
    m = len(rv)
    p = np.zeros(len(amb), np.float64)
    b = 0.0
    use = m >= 2
    if use:
        lx, ly = [], []
        for j in range(m):
            prev = rv[j - 1] if j else 0
            nxt = rv[j + 1] if j + 1 < m else 2 * rv[j] - rv[j - 1]
            Z = 2.0 * float(nr[j]) / float(nxt - prev)
            lx.append(float(log(float(rv[j])))); ly.append(float(log(Z)))
        js = list(range(m))
        if order == "reversed":
            js.reverse()
        elif order == "shuffle":
            np.random.default_rng(shuffle_seed).shuffle(js)
        sx = sy = 0.0
        for j in js:
            sx = sx + lx[j]; sy = sy + ly[j]
        mx, my = sx / float(m), sy / float(m)
        sxy = sxx = 0.0
        for j in js:
            dx = lx[j] - mx
            sxy = sxy + dx * (ly[j] - my); sxx = sxx + dx * dx
        b = sxy / sxx
        use = b < -1.0
    info = {"route": 0 if use else 1, "slope": b, "distinct": m, "active": len(act)}
    if not use:
        den = float(N + len(act))
        for g in act:
            p[g] = float(amb[g] + 1) / den
        return p, info
    rstar = [0.0] * m
    switched = False
    Np = 0.0
    for j in range(m):
        rr = float(rv[j])
        y = rr * math.pow(1.0 + 1.0 / rr, b + 1.0)
        if not switched:
            if j + 1 >= m or rv[j + 1] != rv[j] + 1:
                switched = True
            else:
                rp1, n1, n0r = float(rv[j] + 1), float(nr[j + 1]), float(nr[j])
                x = rp1 * n1 / n0r
                sd = math.sqrt(rp1 * rp1 * (n1 / (n0r * n0r)) * (1.0 + n1 / n0r))
                if abs(x - y) <= 1.96 * sd:
                    switched = True
                else:
                    rstar[j] = x
        if switched:
            rstar[j] = y
        Np = Np + float(nr[j]) * rstar[j]
    P0 = float(nr[0]) / float(N) if rv[0] == 1 and n0 > 0 else 0.0
    where = {x: j for j, x in enumerate(rv)}
    for g in act:
        p[g] = (P0 / float(n0) if n0 else 0.0) if amb[g] == 0 else (1.0 - P0) * rstar[where[amb[g]]] / Np
    return p, info


def thresholds(p, active):
    """T (python ints) as the exact function of p"""
    F = len(p)
    cum, cums, last = 0.0, [], -1
    for g in range(F):
        cum = cum + float(p[g]); cums.append(cum)
        if active[g]:
            last = g
    return np.array([1 << 32 if g >= last else int(cums[g] / cum * 4294967296.0) for g in range(F)], dtype=np.uint64)


def tables(p, active, n_max):
    with np.errstate(divide="ignore"):
        lp = np.where(np.asarray(active, bool), np.log(np.asarray(p, np.float64)), 0.0)
    ln = np.zeros(n_max + 2, np.float64)
    ln[1:] = np.log(np.arange(1, n_max + 2, dtype=np.float64))
    return lp, ln, thresholds(p, active)


def pick(T, u):
    """the first g with u < T[g] (u: uint64 array of 32-bit draws)"""
    return np.searchsorted(np.asarray(T, np.uint64), np.asarray(u, np.uint64), side="right")


def observed(feats, counts, ln, lp):
    o, i = np.float64(0.0), 0
    for g, k in zip(feats, counts):
        for q in range(int(k)):
            i += 1
            o = o + ((ln[i] - ln[q + 1]) + lp[g])
    return o


def simulate(T, lp, ln, n_max, sims, seed, wanted, s_first=0):
    """-> L float64 [len(wanted), sims]: row w = L_s after wanted[w] draws, for the simulations s_first .. s_first + sims - 1"""
    seed &= 0xffffffffffffffff
    key = (seed & 0xffffffff, seed >> 32)
    s = np.arange(s_first, s_first + sims, dtype=np.uint64)
    zero, two = np.zeros(sims, np.uint64), np.full(sims, 2, np.uint64)
    cnt = np.zeros((sims, len(T)), np.int64)
    L = np.zeros(sims, np.float64)
    out = np.zeros((len(wanted), sims), np.float64)
    where = {int(t): w for w, t in enumerate(wanted)}
    rows = np.arange(sims)
    words = None
    for i in range(n_max):
        if i & 3 == 0:
            words = philox4x32_10((np.full(sims, i >> 2, np.uint64), s, zero, two), key)
        g = pick(T, words[i & 3])
        k = cnt[rows, g]
        L = L + ((ln[i + 1] - ln[k + 1]) + lp[g])
        cnt[rows, g] = k + 1
        if i + 1 in where:
            out[where[i + 1]] = L
    return out


def bh(lower, sims, fdr):
    """lower: per candidate in rank order -> (pval, padj, called bool)"""
    m = len(lower)
    pval = np.array([float(int(l) + 1) / float(sims + 1) for l in lower], np.float64)
    by = sorted(range(m), key=lambda j: (int(lower[j]), j))
    padj = np.zeros(m, np.float64)
    run = 1.0
    for pos in range(m, 0, -1):
        j = by[pos - 1]
        run = min(run, min(1.0, float(pval[j]) * float(m) / float(pos)))
        padj[j] = run
    return pval, padj, padj <= fdr


def call(cell_off, feature, count, n_features, params, given=None, keep_sims=False):
    """The whole of br_cellcall -> dict.  given: a dict with p (and optionally lp, ln, T) to use in place of this module's own
    (the GPU tests hand in the object's tables, so everything behind them is compared bit for bit)."""
    P = dict(DEFAULTS, **params)
    off = np.asarray(cell_off, dtype=np.int64)
    feature, count = np.asarray(feature, dtype=np.int64), np.asarray(count, dtype=np.int64)
    K, F = len(off) - 1, int(n_features)
    total, order, rank = totals_and_order(off, count)
    st = total[order]
    thr, n_simple = simple_threshold(st, P["method"], P["expected"], P["percentile"], P["ratio"])
    status = np.zeros(K, np.uint8)
    status[order[:n_simple]] = 1
    R = dict(total=total, order=order, rank=rank, threshold=thr, n_simple=n_simple, status=status, fallback=0, candidates=0)
    if P["method"] != 2 or K == 0:
        return R
    w0, w1 = P["ind_min"], min(P["ind_max"], K)
    if w0 >= w1:
        R["fallback"] = 1
        return R
    amb = np.zeros(F, np.int64)
    for c in order[w0:w1]:
        np.add.at(amb, feature[off[c]:off[c + 1]], count[off[c]:off[c + 1]])
    active = np.zeros(F, np.uint8)
    active[feature] = 1
    R.update(amb=amb, active=active, window=w1 - w0)
    if amb.sum() == 0:
        R["fallback"] = 2
        return R
    med = int(st[n_simple // 2])
    lo = max(P["umi_min"], int(P["umi_frac"] * float(med) + 0.5), 1)
    r1 = min(int(np.sum(st >= lo)), n_simple + P["cand_max"])
    if given is None:
        p, info = sgt(amb, active)
        R["sgt"] = info
    else:
        p = given["p"]
    R.update(p=p, lo=lo)
    if r1 <= n_simple:
        R["fallback"] = 3
        return R
    cand = order[n_simple:r1]
    n_max = int(st[n_simple])
    lp, ln, T = tables(p, active, n_max)
    if given is not None:
        lp, ln, T = given.get("lp", lp), given.get("ln", ln), given.get("T", T)
    wanted = sorted({int(total[c]) for c in cand})
    O = np.array([observed(feature[off[c]:off[c + 1]], count[off[c]:off[c + 1]], ln, lp) for c in cand], np.float64)
    L = simulate(T, lp, ln, n_max, P["sims"], P["seed"], wanted)
    widx = {t: w for w, t in enumerate(wanted)}
    lower = np.array([int(np.sum(L[widx[int(total[c])]] < O[j])) for j, c in enumerate(cand)], np.int64)
    pval, padj, called = bh(lower, P["sims"], P["fdr"])
    status[cand[called]] = 2
    R.update(candidates=len(cand), cand=cand, n_max=n_max, wanted=np.array(wanted, np.int64), lp=lp, ln=ln, T=T, O=O, lower=lower, pval=pval,
             padj=padj, status=status)
    if keep_sims:
        R["L"] = L
    return R

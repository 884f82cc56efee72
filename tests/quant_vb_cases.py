"""The variational Bayes EM of --quant (bramble_amd.h, br_quant, `variational`) restated for the tests, and the inputs its tests
share: the header's digamma series in numpy, the iteration as em_reference of test_quant_cpu.py runs the plain EM's (the same
sequential sums; S summed in transcript order), the six-run spread that says how far the order of a sum and the choice of psi
alone move the result, and three class tables as rows.  Importable without a GPU."""
import functools

import numpy as np

from tests.test_quant_cpu import CHECK_EVERY, MIN_THETA, class_order, classes_of, weights

DIGAMMA_MIN = 1e-10   # e_t = 0 at and below this A_t (salmon's digammaMin)
PSI_THRESHOLD = 16.0  # the recurrence runs until the argument is this or more

# the arguments the digamma checks run on: 200 000 log-uniform draws in [1e-10, 1e9] and the named points
PSI_POINTS = (1e-10, 0.01, 1.0, 1.4616321449683623, 2.0, 6.0, 10.0, 1e9)


def psi_grid():
    rng = np.random.RandomState(20240)
    return np.concatenate([10.0 ** rng.uniform(-10.0, 9.0, size=200000), np.asarray(PSI_POINTS)])


def psi_series(a):
    """psi(a), a > 0, as the header defines it: psi(a) = psi(a + 1) - 1 / a until a >= 16, then
    ln a - 1/(2a) - 1/(12a^2) + 1/(120a^4) - 1/(252a^6) + 1/(240a^8) - 1/(132a^10)"""
    a = np.array(a, dtype=np.float64, copy=True).reshape(-1)
    r = np.zeros_like(a)
    while True:
        m = a < PSI_THRESHOLD
        if not m.any():
            break
        r[m] += 1.0 / a[m]
        a[m] += 1.0
    i = 1.0 / a
    z = i * i
    tail = z * (1.0 / 12.0 - z * (1.0 / 120.0 - z * (1.0 / 252.0 - z * (1.0 / 240.0 - z * (1.0 / 132.0)))))
    return ((np.log(a) - 0.5 * i) - tail) - r


def psi_torch(a):
    import torch
    return torch.special.digamma(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).reshape(-1))).numpy()


def psi_figure(got, ref):
    """the accuracy figure: the largest |got - ref| / max(1, |ref|)"""
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))


def vb_prior(n_tx, lens, prior, per_nucleotide):
    """p_t.  (With "eff_len" the device takes eff_t for the length; the restatement has no fragments and is not run with it.)"""
    if not per_nucleotide:
        return np.full(n_tx, float(prior), dtype=np.float64)
    lens = np.asarray(lens, dtype=np.float64)
    return np.where(lens > 0, float(prior) * lens, 0.0)


def vb_x(alpha, p, w, psi):
    """x_t = exp(psi(A_t) - psi(S)) w_t, A = alpha + p, S the sum of A in transcript order, one by one; 0 where A_t <= 1e-10"""
    A = alpha + p
    S = float(np.cumsum(A)[-1]) if len(A) else 0.0   # (cumsum adds one by one)
    m = A > DIGAMMA_MIN
    if not m.any():
        return np.zeros_like(A)
    e = np.zeros_like(A)
    e[m] = np.exp(psi(A[m]) - psi(np.asarray([S]))[0])
    return e * w


def vb_reference(cl, n_tx, lens=None, length_norm=True, prior=1e-2, per_nucleotide=False, max_iters=10000, tolerance=1e-2, order="forward",
                 psi=psi_torch, sums=None):
    """em_reference with the variational x -> dict theta (the final alpha), tpm, n_iters, rel_change, x (made from the final alpha).
    sums: a list that receives the sum of alpha after every iteration."""
    w = weights(lens, n_tx, length_norm)
    p = vb_prior(n_tx, lens, prior, per_nucleotide)
    n_cls = len(cl["labels"])
    cnt = np.asarray(cl["counts"], dtype=np.float64)
    e_cls = np.asarray([c for c, s in enumerate(cl["labels"]) for _ in s], dtype=np.int64)
    e_tid = np.asarray([t for s in cl["labels"] for t in s], dtype=np.int64)
    rank = np.empty(n_cls, dtype=np.int64)
    rank[class_order(n_cls, order)] = np.arange(n_cls)
    perm = np.argsort(rank[e_cls], kind="stable") if len(e_cls) else np.zeros(0, dtype=np.int64)
    t_cls, t_tid = e_cls[perm], e_tid[perm]
    alpha = np.ones(n_tx, dtype=np.float64)
    it, rel = 0, 0.0
    while it < max_iters:
        it += 1
        x = vb_x(alpha, p, w, psi)
        d = np.bincount(e_cls, weights=x[e_tid], minlength=n_cls) if n_cls else np.zeros(0)
        q = np.where(d > 0, cnt / np.where(d > 0, d, 1.0), 0.0)
        s = np.bincount(t_tid, weights=q[t_cls], minlength=n_tx) if n_cls else np.zeros(n_tx)
        new = x * s
        if sums is not None:
            sums.append(float(new.sum()))
        look = it % CHECK_EVERY == 0 or it == max_iters
        if look:
            m = new > MIN_THETA
            rel = float(np.max(np.abs(new[m] - alpha[m]) / new[m])) if m.any() else 0.0
        alpha = new
        if look and rel < tolerance:
            break
    xw = alpha * w
    tot = 0.0
    for v in xw:   # (transcript order, one by one)
        tot += float(v)
    tpm = 1e6 * xw / tot if tot > 0 else np.zeros(n_tx)
    return {"theta": alpha, "tpm": tpm, "n_iters": it, "rel_change": rel, "x": vb_x(alpha, p, w, psi)}


def posteriors_of(cl, x):
    """x_t / d_c per label entry, d_c summed over the class's labels one after the other (0 where d_c == 0)"""
    out = []
    for s in cl["labels"]:
        d = 0.0
        for t in s:
            d += float(x[t])
        out += [float(x[t]) / d if d != 0.0 else 0.0 for t in s]
    return np.asarray(out, dtype=np.float64)


SIX = tuple((o, f) for f in (psi_torch, psi_series) for o in ("forward", "reversed", 12345))


def vb_spread(cl, n_tx, lens, length_norm, iters, prior=1e-2, per_nucleotide=False):
    """(the forward restatement under torch's psi, s): s = the largest relative difference, over values > 1e-6 of theta and tpm,
    between that run and the five others of {forward, reversed, shuffled class order} x {torch psi, series psi}"""
    runs = [vb_reference(cl, n_tx, lens, length_norm, prior, per_nucleotide, max_iters=iters, tolerance=0, order=o, psi=f) for o, f in SIX]
    s = 0.0
    for key in ("theta", "tpm"):
        ref = runs[0][key]
        m = ref > 1e-6
        for other in runs[1:]:
            s = max(s, float(np.max(np.abs(other[key][m] - ref[m]) / ref[m])))
    return runs[0], s


# ---- the inputs -------------------------------------------------------------------------------------------------------------------
def _tables_of(names, n_tx, lens):
    """names: a list of transcript lists -> the rows as test_gpu_quant.py's _rows_a / _fill take them: every name one alignment"""
    tids = np.asarray([t for nm in names for t in nm], dtype=np.uint32)
    row_off = np.concatenate([[0], np.cumsum([len(nm) for nm in names])]).astype(np.uint64)
    group_off = np.arange(len(names) + 1, dtype=np.uint32)
    return {"tids": tids, "row_off": row_off, "group_off": group_off, "n_tx": n_tx, "lens": lens}


@functools.lru_cache(maxsize=None)
def builder(seed=7, n_names=60000):
    """400 transcripts in genes of 1 to 8 isoforms, lengths 300 .. 5000; n_names names, each a source isoform plus every sibling
    with probability 1/2; and every transcript t a class of its own, {t} with t % 7 + 1 names, so that no two transcripts are
    mirror images of each other (the header's caveat)."""
    rng = np.random.RandomState(seed)
    n_tx = 400
    genes, t = [], 0
    while t < n_tx:
        k = min(int(rng.randint(1, 9)), n_tx - t)
        genes.append(list(range(t, t + k)))
        t += k
    gene_of = np.asarray([g for g, iso in enumerate(genes) for _ in iso])
    lens = rng.randint(300, 5001, size=n_tx).astype(np.int64)
    src = rng.randint(0, n_tx, size=n_names)
    names = []
    for s in src:
        iso = genes[gene_of[s]]
        keep = rng.rand(len(iso)) < 0.5
        names.append([int(s)] + [u for u, kp in zip(iso, keep) if kp and u != s])
    for t in range(n_tx):
        names += [[t]] * (t % 7 + 1)
    return _tables_of(names, n_tx, lens)


@functools.lru_cache(maxsize=None)
def wide():
    """A class of 200 labels and a transcript in 5 000 classes -- what a wave sums -- with small names around them; every
    transcript that has reads also has names of its own, a different number from its neighbours'."""
    rng = np.random.RandomState(3)
    n_tx = 6000
    names = []
    wide_set = rng.permutation(np.arange(100, 700))[:200]
    names.append(list(wide_set))
    names.append(list(rng.permutation(wide_set)))
    names.append(list(wide_set))
    for j in range(5000):
        names.append([1000 + j, 0] if j % 2 else [0, 1000 + j])     # transcript 0 in 5 000 classes
    for j in range(0, 5000, 11):
        names.append([0, 1000 + j])
    for k, t in enumerate(wide_set):
        names += [[int(t)]] * (1 + k % 5)
    for j in range(5000):
        names += [[1000 + j]] * (1 + j % 3)
    names += [[0]] * 40
    names.append([])
    lens = rng.randint(300, 5001, size=n_tx).astype(np.int64)
    return _tables_of(names, n_tx, lens)


@functools.lru_cache(maxsize=None)
def sparse():
    """70 000 transcripts of which 300 have reads: more than 256 block partials in S, and most of S is prior."""
    rng = np.random.RandomState(11)
    n_tx = 70000
    have = np.sort(rng.permutation(n_tx)[:300])
    names = []
    for k, t in enumerate(have):
        names += [[int(t)]] * (1 + k % 9)
        u = int(have[(k + 1 + k % 4) % 300])
        names += [[int(t), u]] * (2 + k % 5)
    for _ in range(400):
        names.append([int(v) for v in rng.choice(have, size=3, replace=False)])
    lens = rng.randint(300, 5001, size=n_tx).astype(np.int64)
    return _tables_of(names, n_tx, lens)


@functools.lru_cache(maxsize=None)
def classes(which):
    tb = {"builder": builder, "wide": wide, "sparse": sparse}[which]()
    return classes_of(tb["tids"], tb["row_off"], tb["group_off"])


# (input, length_norm, prior, per_nucleotide) of the GPU tests' value runs: the builder pe-style with lengths and ont-style
# without, the two hand-built tables, and the prior per nucleotide for the length-normalised case only
VALUE_CASES = [("builder", 1, 1e-2, 0), ("builder", 0, 1e-2, 0), ("wide", 0, 1e-2, 0), ("sparse", 0, 1e-2, 0), ("builder", 1, 1e-5, 1)]
VALUE_ITERS = 200
STOP_CASE = ("builder", 1, 1e-2, 0)   # the stopping test's input: default tolerance
BOOT_CASE = ("builder", 1, 1e-2, 0)
BOOT_SEED, BOOT_B, BOOT_ITERS = 5, 7, 200


@functools.lru_cache(maxsize=None)
def spread_of(which, length_norm, prior, per_nucleotide, iters=VALUE_ITERS):
    tb = {"builder": builder, "wide": wide, "sparse": sparse}[which]()
    return vb_spread(classes(which), tb["n_tx"], tb["lens"], bool(length_norm), iters, prior, bool(per_nucleotide))


@functools.lru_cache(maxsize=None)
def boot_spreads(seed=BOOT_SEED, n_boot=BOOT_B):
    """per replicate of BOOT_CASE (the forward restatement under torch's psi on boot_counts' counts, its own six-run spread)"""
    from tests.test_quant_boot_cpu import boot_counts
    which, length_norm, prior, per_nt = BOOT_CASE
    tb, cl = builder(), classes(which)
    out = []
    for b in range(n_boot):
        cl_b = dict(cl, counts=[int(v) for v in boot_counts(cl["counts"], seed, b)])
        out.append(vb_spread(cl_b, tb["n_tx"], tb["lens"], bool(length_norm), BOOT_ITERS, prior, bool(per_nt)))
    return out

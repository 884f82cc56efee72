"""Inputs and numpy references for the probes of cigar_inl.h and wave_turns (test_gpu_cigar_probe.py runs them on the device,
test_cigar_ref_cpu.py shows that they tell a right table from a wrong one).  Nothing here is taken from the code under test:
the op codes are the BAM specification's (M I D N S H P = X: 0 .. 8)."""
import functools

import numpy as np

REF_CODES = (0, 2, 3, 7, 8)     # M D N = X consume the reference
COVER_CODES = (0, 7, 8)         # M = X
SKIP_CODES = (2, 3)             # D N
MAX_LEN = (1 << 28) - 1         # the longest op a 32-bit word holds
CIGAR_SIZES = (0, 1, 63, 64, 65, 128, 300)


def op_words(codes, lens):
    return (np.asarray(lens, dtype=np.uint32) << np.uint32(4)) | np.asarray(codes, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def pool_case(seed=7):
    """(pool, offs, ns): CIGARs of CIGAR_SIZES ops, all 16 codes with lengths up to MAX_LEN, each at an odd offset of one pool,
    random words between them.  The 300-op CIGAR holds an M of MAX_LEN bases; the sums of the long ones pass 2^32."""
    rng = np.random.default_rng(seed)
    parts, offs, at = [], [], 0
    for n in CIGAR_SIZES:
        gap = int(rng.integers(1, 9))
        gap += (at + gap + 1) % 2        # the CIGAR begins at an odd word
        parts.append(rng.integers(0, 1 << 32, gap, dtype=np.uint64).astype(np.uint32))
        at += gap
        offs.append(at)
        # (every other op consumes the reference for certain: 63 ops of 27 bits on average pass 2^32 then)
        codes = np.where(rng.random(n) < 0.5, rng.choice(REF_CODES, n), rng.integers(0, 16, n))
        ops = op_words(codes, rng.integers(0, MAX_LEN + 1, n))
        if n == 300:
            ops[100:116] = op_words(np.arange(16), rng.integers(1, MAX_LEN + 1, 16))     # every code is there
            ops[150] = op_words([0], [MAX_LEN])[0]
        # the first and the last op, and the words in front of and behind the CIGAR, consume the reference: a walk that is an
        # op off at either end gives another sum
        edge = op_words(rng.choice(REF_CODES, 4), rng.integers(1, MAX_LEN + 1, 4))
        parts[-1][-1] = edge[0]
        if n >= 2:
            ops[0], ops[-1] = edge[1], edge[2]
        parts.append(np.append(ops, edge[3]))
        at += n + 1
    parts.append(rng.integers(0, 1 << 32, 5, dtype=np.uint64).astype(np.uint32))
    return np.concatenate(parts), np.asarray(offs, dtype=np.uint64), np.asarray(CIGAR_SIZES, dtype=np.uint32)


def ref_len_sums(pool, offs, ns, codes=REF_CODES):
    """per CIGAR: the bases of its ops whose code is in `codes`, exact (uint64; 300 ops of 28 bits stay far below 2^64)"""
    out = np.zeros(len(offs), dtype=np.uint64)
    for i, (o, n) in enumerate(zip(offs.tolist(), ns.tolist())):
        w = pool[o:o + n]
        out[i] = (w[np.isin(w & np.uint32(15), codes)] >> np.uint32(4)).astype(np.uint64).sum(dtype=np.uint64)
    return out


@functools.lru_cache(maxsize=None)
def table_ops(seed=11):
    """16 op words, code t in word t, every length positive and with bits above the low four (a table indexed by the whole
    word, or by its length, would show)"""
    rng = np.random.default_rng(seed)
    return op_words(np.arange(16), rng.integers(1 << 8, MAX_LEN + 1, 16))


def table_ref(ops, codes=REF_CODES):
    """(tab, tab_len, inl) as k_probe_cigar leaves them: covers | skips << 1, the reference bases of each word, and those of the
    first n = 0, 1, 2 ops of (ops[t], ops[t + 1 mod 16])"""
    code, length = ops & np.uint32(15), (ops >> np.uint32(4)).astype(np.uint64)
    tab = np.isin(code, COVER_CODES).astype(np.uint32) | (np.isin(code, SKIP_CODES).astype(np.uint32) << np.uint32(1))
    tab_len = np.where(np.isin(code, codes), length, np.uint64(0)).astype(np.uint64)
    inl = np.zeros(48, dtype=np.uint64)
    inl[1::3] = tab_len
    inl[2::3] = tab_len + np.roll(tab_len, -1)
    return tab, tab_len, inl


def pool_holds_cases(n_pool_words):
    """(off, n, expected): the escapes of test_gpu_coverage.py's refused adds, and the fits next to them"""
    P = int(n_pool_words)
    return [(P + 1, 300, False), (2 ** 64 - 100, 300, False), (P - 299, 300, False), (P - 63, 64, False), (1 << 40, 64, False),
            (P + 1, 0, False), (2 ** 64 - 1, 1, False), (2 ** 64 - 1, 0, False), (0, P + 1, False),
            (P - 300, 300, True), (P - 64, 64, True), (0, P, True), (P, 0, True), (0, 0, True), (1, 3, True)]


# ---- wave_turns ----
NONE, ALL, LANE0, LANE63, EVEN, ODD = 0, (1 << 64) - 1, 1, 1 << 63, 0x5555555555555555, 0xaaaaaaaaaaaaaaaa


def turn_cases(seed=3):
    """name -> the masks of a block's four waves: all different in every case; each of none, all 64, lane 0 only, lane 63 only
    and alternating lanes somewhere, and one random mask in every wave"""
    rng = np.random.default_rng(seed)
    rnd = [int(x) for x in rng.integers(0, 1 << 64, 4, dtype=np.uint64)]
    return {"edges": (NONE, ALL, LANE0, LANE63), "edges moved": (LANE63, LANE0, EVEN, ODD), "alternating": (ODD, NONE, ALL, EVEN),
            "random": tuple(rnd)}


def turn_inputs(masks, seed=5):
    """(flag, val): 256 words each; a set flag is any nonzero word"""
    rng = np.random.default_rng(seed)
    bits = np.array([(m >> l) & 1 for m in masks for l in range(64)], dtype=np.uint32)
    flag = bits * rng.integers(1, 1 << 32, 256, dtype=np.uint64).astype(np.uint32)
    return flag, rng.integers(0, 1 << 32, 256, dtype=np.uint64).astype(np.uint32)


def turn_ref(masks, val, fill):
    """(lists, counts): per wave its set lanes in ascending order as (lane, that lane's value, 64 lanes in the call), `fill`
    behind them"""
    lists = np.full((4, 64, 3), fill, dtype=np.uint32)
    counts = np.zeros(4, dtype=np.uint32)
    for w, m in enumerate(masks):
        lanes = [l for l in range(64) if (m >> l) & 1]
        counts[w] = len(lanes)
        for k, l in enumerate(lanes):
            lists[w, k] = (l, val[64 * w + l], 64)
    return lists.reshape(-1), counts

"""References, wrong variants and inputs for the tests of the shared scan unit and the wave primitives
(scan_kernels.hip, wave_inl.h, launch_scan3).

The references restate each operation from its definition in Python integers or plain NumPy.  The wrong variants are the
ways a scan kernel goes wrong; test_scan_ref_cpu.py shows that the inputs below tell every one of them from the reference,
so that equality on the GPU (test_gpu_scan_unit.py) means something.  Nothing here touches a GPU.
"""
from itertools import accumulate

import numpy as np

# the shape of the scan unit (scan_kernels.h): 256 threads x 8 items a tile, up to 4 tiles in one launch, 2 048 tile sums a
# round of the one-block pass over the tile sums
TILE = 2048
ONE_LAUNCH = 4 * TILE
ROUND_SUMS = 2048
ROUND_ITEMS = ROUND_SUMS * TILE           # 4 194 304: more items than this run a second round of k_scan_top

SCAN_SIZES = (0, 1, 7, 8, 9, 2047, 2048, 2049, 8191, 8192, 8193, 70001, 4194304, 4194305, 4200003)
SCAN3_SIZES = (0, 1, 1024, 1025, 2048, 8192, 8193, 70001, 4194305)
TOP8_SIZES = (1, 255, 2047, 2048, 2049, 4097, 5000)        # scan_top_rounds<1, 8> and <3, 8>: 2 048 sums a round
TOP32_SIZES = (1, 8191, 8192, 8193, 20000)                 # scan_top_rounds<1, 32>: 8 192 sums a round
ALIGN_SIZES = (9, 2049, 8193, 70001)
COPY8_SIZES = (0, 1, 7, 8, 9, 15, 2047, 2048, 2049, 8191)   # load8 / store8: around a thread's eight items and around a tile
BOUNDARIES = (7, 8, 2047, 2048, 8191, 8192, ROUND_ITEMS - 1, ROUND_ITEMS)
WIDTHS = (8, 16, 32, 64)
EXACT_UP_TO = 100000      # above this many items the references use wrapping uint64 sums instead of Python integers

_DT = {32: np.uint32, 64: np.uint64}


# ---------------------------------------------------------------------------------------------------------------------
# references
# ---------------------------------------------------------------------------------------------------------------------

def sums_mod64(values):
    """out[i] = values[0] + ... + values[i - 1] for i in [0, n] in wrapping uint64 arithmetic: uint64 addition in NumPy wraps,
    which is addition modulo 2^64, and reduction modulo 2^64 commutes with sums.  test_scan_ref_cpu.py checks it against
    excl_scan_exact."""
    v = np.asarray(values).astype(np.uint64)
    out = np.zeros(v.size + 1, dtype=np.uint64)
    np.cumsum(v, dtype=np.uint64, out=out[1:])
    return out


def excl_scan_exact(values, bits):
    """out[i] = values[0] + ... + values[i - 1] for i in [0, n], in Python integers, reduced modulo 2^bits at the end;
    returns (out, the unreduced total)"""
    sums = [0]
    sums.extend(accumulate(int(v) for v in np.asarray(values).tolist()))
    mask = (1 << bits) - 1
    return np.array([s & mask for s in sums], dtype=_DT[bits]), sums[-1]


def excl_scan_wrapping(values, bits):
    """The same for large n, from sums_mod64 (reduced further modulo 2^32 where asked); the total is exact as long as
    n * max < 2^64, which is asserted."""
    v = np.asarray(values)
    assert v.size == 0 or int(v.max()) * v.size < 1 << 64
    out = sums_mod64(v)
    return (out if bits == 64 else out.astype(np.uint32)), int(out[-1])


def excl_scan(values, bits):
    n = np.asarray(values).size
    return excl_scan_exact(values, bits) if n <= EXACT_UP_TO else excl_scan_wrapping(values, bits)


def scan3_values(n_matches, class_word, cigar_off=None, ideal_cap=None):
    """scan3_value of project_kernels.hip, per alignment: (n_matches, n_matches * CIGAR slot capacity, n_matches if the
    alignment is of the simple class).  The capacity is the class word's low 31 bits, or with the -S capacities
    (cigar_off[i + 1] - cigar_off[i]) + 2 * ideal_cap[i] in 32-bit arithmetic.  Alignments without matches count nothing."""
    nm = np.asarray(n_matches).astype(np.uint64)
    cf = np.asarray(class_word).astype(np.uint64)
    cap = cf & np.uint64(0x7fffffff)
    if ideal_cap is not None:
        co = np.asarray(cigar_off).astype(np.uint64)
        cap = (co[1:] - co[:-1] + np.uint64(2) * np.asarray(ideal_cap).astype(np.uint64)) & np.uint64(0xffffffff)
    assert nm.size == 0 or (int(nm.max()) < 1 << 32 and int(cap.max()) < 1 << 32)   # the product below is exact in 64 bits
    simple = (cf >> np.uint64(31)) != 0
    return nm, nm * cap, np.where(simple, nm, np.uint64(0))


def scan3_ref(n_matches, class_word, cigar_off=None, ideal_cap=None):
    """-> (match_off u32[n + 1], cig_base u64[n + 1], fast_pre u32[n + 1], the three totals modulo 2^64)"""
    v = scan3_values(n_matches, class_word, cigar_off, ideal_cap)
    outs, tots = [], []
    for c, bits in enumerate((32, 64, 32)):
        full = excl_scan_exact(v[c], 64)[0] if v[c].size <= EXACT_UP_TO else sums_mod64(v[c])
        tots.append(int(full[-1]))
        outs.append(full if bits == 64 else full.astype(np.uint32))   # the 32-bit outputs are the low words of the exact sums
    return outs[0], outs[1], outs[2], np.array(tots, dtype=np.uint64)


def top_rounds_ref(tile_sums, channels):
    """scan_top_rounds: `channels` arrays of n_tiles sums, one behind the other, each scanned exclusively in place (modulo
    2^64), and the total of each -> (scanned arrays, totals)"""
    t = np.asarray(tile_sums, dtype=np.uint64).reshape(channels, -1)
    out = np.empty_like(t)
    tots = np.empty(channels, dtype=np.uint64)
    for c in range(channels):
        full, _ = excl_scan_exact(t[c], 64)
        out[c], tots[c] = full[:-1], full[-1]
    return out.reshape(-1), tots


def copy8_ref(values):
    """the load8 / store8 probe: every item complemented; per thread the sum of its eight items, items at or past n being 0"""
    v = np.asarray(values)
    tiles = max((v.size + TILE - 1) // TILE, 1)
    padded = np.zeros(tiles * TILE, dtype=np.uint64)
    padded[:v.size] = v
    return ~v, padded.reshape(-1, 8).sum(axis=1, dtype=np.uint64)


def _groups(v, w):
    v = np.asarray(v)
    assert v.size % w == 0
    return v.reshape(-1, w)


def group_scan(v, w):
    """wave_scan<T, W>: the inclusive prefix sum over each group of w consecutive lanes, in the type's own arithmetic"""
    g = _groups(v, w)
    return np.cumsum(g, axis=1, dtype=g.dtype).reshape(-1)


_REDUCE = {"sum": lambda g: np.add.reduce(g, axis=1, dtype=g.dtype), "max": lambda g: g.max(axis=1), "min": lambda g: g.min(axis=1),
           "or": lambda g: np.bitwise_or.reduce(g, axis=1), "and": lambda g: np.bitwise_and.reduce(g, axis=1)}


def group_reduce(op, v, w):
    """wave_sum / max / min / or / and <T, W> for integers: every lane of a group holds the group's reduction"""
    g = _groups(v, w)
    return np.repeat(_REDUCE[op](g), w).astype(g.dtype)


def butterfly_sum(v, w, order="down"):
    """wave_sum<double, W>: for d = w / 2 ... 1, v[i] += v[i ^ d] for all lanes at once, in float64 (IEEE addition, nothing
    contracted: exact restatement).  order "up" is the wrong order d = 1 ... w / 2."""
    g = _groups(np.asarray(v, dtype=np.float64), w).copy()
    lanes = np.arange(w)
    ds = [w >> (k + 1) for k in range(w.bit_length() - 1)]
    for d in (ds if order == "down" else ds[::-1]):
        g = g + g[:, lanes ^ d]
    return g.reshape(-1)


def left_to_right_sum(v, w):
    """a wrong order for wave_sum<double>: lane 0 + lane 1 + ... in sequence, in every lane"""
    g = _groups(np.asarray(v, dtype=np.float64), w)
    acc = g[:, 0].copy()
    for k in range(1, w):
        acc = acc + g[:, k]
    return np.repeat(acc, w)


def block_scan_ref(v):
    """block_excl_scan_256: per block of 256 the exclusive prefix sums and the block's total (in every thread)"""
    g = _groups(v, 256)
    inc = np.cumsum(g, axis=1, dtype=g.dtype)
    return (inc - g).reshape(-1), np.repeat(inc[:, -1], 256)


def block_bits_ref(o, a):
    """block_bits: out[2 * block] = OR of o, out[2 * block + 1] = AND of a over the block's 256 threads"""
    out = np.empty(2 * (np.asarray(o).size // 256), dtype=np.uint64)
    out[0::2] = np.bitwise_or.reduce(_groups(o, 256), axis=1)
    out[1::2] = np.bitwise_and.reduce(_groups(a, 256), axis=1)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# wrong variants: each takes the values and returns (out, total) as a kernel with that mistake would
# ---------------------------------------------------------------------------------------------------------------------

def _cut(c, bits):
    return c if bits == 64 else c.astype(np.uint32)


def wrong_inclusive(values, bits):
    c = sums_mod64(values)
    out = c.copy()
    out[:-1] = c[1:]
    return _cut(out, bits), int(c[-1])


def wrong_no_last(values, bits, prefill):
    """out[n] (and the total) never written: they keep what the buffer held"""
    c = sums_mod64(values)
    c[-1] = prefill & ((1 << bits) - 1)
    return _cut(c, bits), prefill


def wrong_carry_dropped(values, bits, at):
    """the sum of the first `at` items is not carried into what follows (a tile, launch or round boundary)"""
    c = sums_mod64(values)
    if c.size - 1 > at:
        c[at:] -= c[at]
    return _cut(c, bits), int(c[-1])


def wrong_carry32(values, bits, step):
    """the carry from one piece of `step` items into the next is kept in 32 bits"""
    v = np.asarray(values).astype(np.uint64)
    out = np.zeros(v.size + 1, dtype=np.uint64)
    carry = 0
    for s in range(0, max(v.size, 1), step):
        piece = sums_mod64(v[s:s + step])
        out[s:s + piece.size] = piece + np.uint64(carry)
        carry = (carry + int(piece[-1])) & 0xffffffff
    return _cut(out, bits), int(out[-1])


def scan_variants(values, bits, boundaries, step, prefill):
    """name -> (out, total) of every wrong variant that applies at this size"""
    n = np.asarray(values).size
    wrong = {}
    if n >= 1:
        wrong["inclusive"] = wrong_inclusive(values, bits)
    wrong["out[n] missing"] = wrong_no_last(values, bits, prefill)
    for name, at in boundaries.items():
        if n > at:
            wrong["carry dropped at " + name] = wrong_carry_dropped(values, bits, at)
    if n > step:
        wrong["32-bit carry"] = wrong_carry32(values, bits, step)
    return wrong


def scan3_swapped(ref):
    """the channels of the three-value scan in another order: what lands in match_off is fast_pre's and so on"""
    mo, cb, fp, tot = ref
    return [(fp, cb, mo, tot[[2, 1, 0]]), (cb.astype(np.uint32), mo.astype(np.uint64), fp, tot[[1, 0, 2]]),
            (mo, fp.astype(np.uint64), cb.astype(np.uint32), tot[[0, 2, 1]])]


# ---------------------------------------------------------------------------------------------------------------------
# inputs (the GPU tests run exactly these; the CPU tests show that they separate the variants)
# ---------------------------------------------------------------------------------------------------------------------

def _rng(*key):
    return np.random.default_rng([20240611, *key])


def _u64(r, n):
    return r.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + r.integers(0, 2, n, dtype=np.uint64)


def scan_inputs_u32(n):
    """launch_scan from u32: uniform random over the full range (the u32 output wraps many times, the total passes 2^32 within
    a few items), all ones (out[i] == i shows a misplaced item by its index), a single 1 at each boundary index and at n - 1"""
    sets = {"random": _rng(1, n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), "ones": np.ones(n, dtype=np.uint32)}
    for at in sorted({b for b in BOUNDARIES if b < n} | ({n - 1} if n else set())):
        v = np.zeros(n, dtype=np.uint32)
        v[at] = 1
        sets["single@%d" % at] = v
    return sets


def scan_inputs_u64(n):
    """launch_scan in place: random values below 2^40 (the carries cross 2^32 at once), and all ones"""
    return {"random": _rng(2, n).integers(0, 1 << 40, n, dtype=np.uint64), "ones": np.ones(n, dtype=np.uint64)}


def top_inputs(n_tiles, channels):
    """tile sums for scan_top_rounds: values up to 2^40, so the carries cross 2^32"""
    return _rng(3, n_tiles, channels).integers(0, (1 << 40) + 1, n_tiles * channels, dtype=np.uint64)


def scan3_inputs(n, with_caps, first_simple=True):
    """n_matches in 0 ... 5 000 with about half of them zero; class words with capacities up to 2^31 - 1 and the top bit
    random; with_caps: the -S capacities too (CIGAR lengths up to 1 000 ops, ideal capacities up to 2^20).

    The first two alignments are pinned, so that no channel is all zeros and no two channels are alike at any n >= 2: both have
    matches (in different numbers) and a capacity above 1, the first is of the simple class (or not: first_simple) and the
    second of the other."""
    r = _rng(4, n, int(with_caps))
    nm = (r.integers(0, 5001, n, dtype=np.uint64) * r.integers(0, 2, n, dtype=np.uint64)).astype(np.uint32)
    # (the top bit set in 7 of 8: at the largest size the simple-class total passes 2^32 too, which is where a carry kept in 32
    # bits shows in a 32-bit output's total)
    cf = (r.integers(0, 1 << 31, n, dtype=np.uint64) | (np.minimum(r.integers(0, 8, n, dtype=np.uint64), 1) << np.uint64(31))).astype(np.uint32)
    co = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(r.integers(0, 1001, n, dtype=np.uint64), out=co[1:])
    assert int(co[-1]) < 1 << 32
    ic = r.integers(0, (1 << 20) + 1, n, dtype=np.uint64).astype(np.uint32)
    for k in range(min(n, 2)):
        nm[k] = 1 + int(nm[0]) % 4999 + k                    # 1 ... 4 999, then one more
        simple = first_simple == (k == 0)
        cf[k] = (int(cf[k]) & 0x7fffffff) | 2 | (int(simple) << 31)    # capacity >= 2 from the class word
        ic[k] = max(int(ic[k]), 1)                           # and >= 2 from the -S capacities
    return (nm, cf, co.astype(np.uint32), ic) if with_caps else (nm, cf, None, None)


def scan3_input_sets(n, with_caps):
    """name -> inputs of launch_scan3 at this size.  One set from n = 2 on.  A single alignment's simple-class count is either
    its match count or zero, so at n = 1 no one set can tell both an inclusive fast_pre and fast_pre and match_off swapped from
    the reference: there are two sets, one of each class, which do so between them."""
    if n == 1:
        return {"simple": scan3_inputs(1, with_caps, True), "general": scan3_inputs(1, with_caps, False)}
    return {"random": scan3_inputs(n, with_caps)}


def wave_edges(w):
    """the threads of a block at the edges of the lane groups"""
    return (0, w - 1, w, 255)


def wave_inputs(dtype, w, n_blocks=4):
    """4 blocks of 256 lanes: random values; zeros with one value in block j's thread wave_edges(w)[j]; all ones with one
    cleared bit in the same places"""
    dtype = np.dtype(dtype)
    bits = dtype.itemsize * 8
    n = 256 * n_blocks
    r = _rng(5, bits, w)
    sets = {"random": _u64(r, n).astype(dtype)}
    one = np.zeros(n, dtype=dtype)
    clear = np.full(n, (1 << bits) - 1, dtype=dtype)
    for j, k in enumerate(wave_edges(w)):
        one[(j % n_blocks) * 256 + k] = dtype.type(1 << ((5 * j + 3) % bits))
        clear[(j % n_blocks) * 256 + k] = dtype.type(((1 << bits) - 1) ^ (1 << ((7 * j + 1) % bits)))
    sets["one set"] = one
    sets["one cleared"] = clear
    return sets


def wave_doubles(w, n_blocks=4):
    """mixed magnitudes and signs: the bits of a sum depend on its order"""
    r = _rng(6, w)
    n = 256 * n_blocks
    return r.standard_normal(n) * np.power(10.0, r.integers(-8, 9, n))


def block_bits_inputs(n_blocks=8):
    """o, a for block_bits: random blocks, then blocks whose only set bit of o (only cleared bit of a) sits in thread 0, 63, 64
    or 255"""
    n = 256 * n_blocks
    r = _rng(7)
    # a block's values share a random mask, so that its OR and AND are neither all ones nor all zeros
    o = _u64(r, n) & np.repeat(_u64(r, n_blocks), 256)
    a = _u64(r, n) | np.repeat(_u64(r, n_blocks), 256)
    for j, k in enumerate((0, 63, 64, 255)):
        b = n_blocks - 4 + j
        o[b * 256:(b + 1) * 256] = 0
        a[b * 256:(b + 1) * 256] = np.uint64(0xffffffffffffffff)
        o[b * 256 + k] = np.uint64(1 << (11 * j + 9))
        a[b * 256 + k] = np.uint64(0xffffffffffffffff ^ (1 << (13 * j + 20)))
    return o, a

"""A bigWig writer for the tests: the layout and the definitions of include/bramble_amd.h (br_coverage_bigwig) restated in numpy and
Python integers, from what tests.test_coverage_cpu.coverage_of gives (the depth per transcript and the runs).  It writes the
uncompressed form and, through zlib.compress, the compressed one; sums are exact integers rounded once.  Beside it the names case
of the tests and the bound helpers."""
import functools
import math
import struct
import zlib
from fractions import Fraction

import numpy as np

from tests.bigwig_ref import BIGWIG_MAGIC, CHROM_MAGIC, RTREE_MAGIC, ZOOM, levels_of

DEFAULTS = {"items_per_slot": 1024, "block_size": 256, "zoom_levels": 4, "first_reduction": 32, "compress": 1}

# eleven names for the transcripts of the hand-built table: @SQ order is not byte order ("t10" < "t1a" < "t2", upper case in front
# of lower), lengths 1 and 40, and -- with that table -- transcripts without runs between ones with runs
NAMES_CASE = ["t1a", "t10", "t1", "unused-a", "unused-b", "T2", "x", "t" * 40, "t2", "unused-c", "A"]


def hand_built():
    """the hand-built table of tests/test_gpu_coverage.py: (rows, its coverage, the lengths); NAMES_CASE names its transcripts"""
    from tests.test_gpu_coverage import HAND_LENS, _hand_built
    rows, (cov, _) = _hand_built()
    return rows, cov, HAND_LENS


@functools.lru_cache(maxsize=None)
def boundary_case(n_runs, random_depth):
    """One transcript with exactly n_runs runs.  Periodic: every base its own run, depth 1, 2, 1, ... (unit weight).  Random: runs of
    1 .. 40 bases, 1 .. 40 bases apart from base 300 on, two rows of weight nh on each with NH drawn from 2 .. 255: the sum of the
    two weights fills the float's 24 bits, and starts, ends and values are pseudo-random bytes with few repeats.  -> (rows, nh per row or None, the coverage, the lengths, wide)"""
    from tests.test_coverage_cpu import coverage_of
    from tests.test_coverage_weight_cpu import weight_words_nh, weighted_coverage_of
    from tests.test_quant_fld_cpu import rows_of
    if not random_depth:
        lens = np.asarray([n_runs], dtype=np.int64)
        rows = rows_of([(0, 0, 0, "%dM" % n_runs)] + [(0, p, 0, "1M") for p in range(1, n_runs, 2)])
        return rows, None, coverage_of(rows, lens), lens, False
    rng = np.random.RandomState(n_runs)
    length, gap, nh = rng.randint(1, 41, n_runs), rng.randint(1, 41, n_runs), rng.randint(2, 256, 2 * n_runs)
    start = 300 + np.cumsum(length + gap) - length
    lens = np.asarray([int(start[-1] + length[-1]) + 3], dtype=np.int64)
    rows = rows_of([(0, int(s), 0, "%dM" % n) for s, n in zip(start, length) for _ in range(2)])
    return rows, nh, weighted_coverage_of(rows, lens, weight_words_nh(nh)), lens, True


ZOOM_EDGE_NAMES = ["len31", "len32", "len33", "len2049", "len5"]


@functools.lru_cache(maxsize=None)
def zoom_edge_case():
    """lengths 31, 32, 33 and 2049 and one of 5 (shorter than every R); coverage only in a window's last base; windows without
    coverage between covered ones.  -> (rows, the coverage, the lengths)"""
    from tests.test_coverage_cpu import coverage_of
    from tests.test_quant_fld_cpu import rows_of
    lens = np.asarray([31, 32, 33, 2049, 5], dtype=np.int64)
    rows = rows_of([(0, 30, 0, "1M"), (1, 31, 0, "1M"), (1, 0, 0, "2M"), (2, 32, 0, "1M"), (2, 0, 0, "3M"), (3, 2048, 0, "1M"), (3, 127, 0, "1M"),
                    (3, 600, 0, "40M"), (3, 610, 0, "5M"), (4, 1, 0, "3M")])
    return rows, coverage_of(rows, lens), lens


def f32_exact(num, shift):
    """the float32 nearest (ties to even) to num * 2^-shift, num a non-negative Python integer"""
    if num == 0:
        return np.float32(0)
    e = max(num.bit_length() - 24, 0)
    q = num >> e
    if e:
        r, half = num & ((1 << e) - 1), 1 << (e - 1)
        if r > half or (r == half and (q & 1)):
            q += 1
    return np.float32(math.ldexp(float(q), e - shift))


def value_of(depth, wide):
    """the float32 value of a depth word: (float) depth, or (float) ((double) depth64 * 2^-32)"""
    return np.float32(np.float64(np.uint64(depth)) * 2.0 ** -32) if wide else np.float32(np.uint32(depth))


def _tree(n, block_size, leaf_item, inner_item, leaf_bytes, inner_bytes, at):
    """the nodes of a tree over n items, root level first: leaf_bytes(i) / inner_bytes(level, i, child offset) give an item"""
    bs, items = levels_of(n, block_size)
    size = [4 + bs * (leaf_item if l == 0 else inner_item) for l in range(len(items))]
    nodes = [max(-(-m // bs), 1) for m in items]
    start, p = {}, at
    for l in range(len(items) - 1, -1, -1):
        start[l] = p
        p += nodes[l] * size[l]
    out = b""
    for l in range(len(items) - 1, -1, -1):
        for k in range(nodes[l]):
            idx = range(k * bs, min((k + 1) * bs, items[l]))
            body = b"".join(leaf_bytes(i) if l == 0 else inner_bytes(l, i, start[l - 1] + i * size[l - 1]) for i in idx)
            out += struct.pack("<BBH", 1 if l == 0 else 0, 0, len(idx)) + body + b"\0" * (size[l] - 4 - len(body))
    return bs, out


def _rtree(bounds, where, data_base, block_size, at):
    """bounds: [(lo, hi)] with lo / hi = (chrom, base); item i lies at data_base + where[i]; the data ends at `at`, where the tree begins"""
    n = len(bounds)
    bs, items = levels_of(n, block_size)
    level = {0: bounds}
    for l in range(1, len(items)):
        b = level[l - 1]
        level[l] = [(min(x[0] for x in b[i:i + bs]), max(x[1] for x in b[i:i + bs])) for i in range(0, len(b), bs)]

    def four(l, i):
        lo, hi = level[l][i]
        return struct.pack("<IIII", lo[0], lo[1], hi[0], hi[1])
    _, body = _tree(n, block_size, 32, 24, lambda i: four(0, i) + struct.pack("<QQ", data_base + where[i], where[i + 1] - where[i]),
                    lambda l, i, child: four(l, i) + struct.pack("<Q", child), at + 48)
    top = level[len(items) - 1]
    lo, hi = (min(x[0] for x in top), max(x[1] for x in top)) if n else ((0, 0), (0, 0))
    return struct.pack("<IIQIIIIQII", RTREE_MAGIC, bs, n, lo[0], lo[1], hi[0], hi[1], at, 1, 0) + body


def zoom_records(depth, lens, chrom_tids, R, wide):
    """the records of one zoom level (a ZOOM array) and, beside each, the exact sums (sum of depth, sum of depth^2) as integers"""
    rec, exact = [], []
    for cid, t in enumerate(chrom_tids):
        d, L = depth[t], int(lens[t])
        for w in range(-(-L // R)):
            seg = [int(x) for x in d[w * R:(w + 1) * R] if x]
            if not seg:
                continue
            s1, s2 = sum(seg), sum(x * x for x in seg)
            rec.append((cid, w * R, min((w + 1) * R, L), len(seg), value_of(min(seg), wide), value_of(max(seg), wide),
                        f32_exact(s1, 32 if wide else 0), f32_exact(s2, 64 if wide else 0)))
            exact.append((s1, s2))
    return np.asarray(rec, dtype=ZOOM), exact


def chromosomes(runs, names):
    """the transcripts with runs in the byte order of their names: [tid] by chromId"""
    with_runs = sorted(set(int(t) for t in runs[0]))
    return sorted(with_runs, key=lambda t: names[t].encode())


def total_summary(depth, chrom_tids, wide):
    """(validCount, min, max, sum, sum of squares) over all covered bases: exact, each rounded once to double"""
    n = s1 = s2 = 0
    mn, mx = None, 0
    for t in chrom_tids:
        seg = [int(x) for x in depth[t] if x]
        n += len(seg); s1 += sum(seg); s2 += sum(x * x for x in seg)
        mn = min(seg) if mn is None else min(mn, min(seg)); mx = max(mx, max(seg))
    if not n:
        return 0, 0.0, 0.0, 0.0, 0.0
    k = 32 if wide else 0
    return n, float(Fraction(mn, 1 << k)), float(Fraction(mx, 1 << k)), float(Fraction(s1, 1 << k)), float(Fraction(s2, 1 << (2 * k)))


def write_bigwig(cov, lens, names, wide=False, **opts):
    """cov: depth (an integer array per transcript) and runs (tid, start, end, depth) as coverage_of gives them (wide: the words are
    uint64 in units of 2^-32).  -> (the file's bytes, {"zoom_exact": per level the exact sums of its records})"""
    o = dict(DEFAULTS)
    o.update({k: v for k, v in opts.items() if v})
    S, bs_opt, R0 = o["items_per_slot"], o["block_size"], o["first_reduction"]
    Z = 0 if o["zoom_levels"] < 0 else o["zoom_levels"]
    compress = o["compress"] >= 0
    pack = zlib.compress if compress else (lambda b: b)
    tid, start, end, dep = [np.asarray(v) for v in cov["runs"]]
    chrom_tids = chromosomes(cov["runs"], names)
    enc = [names[t].encode() for t in chrom_tids]
    assert all(enc) and len(set(enc)) == len(enc)
    ks = max([len(e) for e in enc] + [0])
    head_bytes = 64 + 24 * Z + 40
    _, ctree_nodes = _tree(len(enc), bs_opt, ks + 8, ks + 8,
                           lambda i: enc[i].ljust(ks, b"\0") + struct.pack("<II", i, int(lens[chrom_tids[i]])),
                           lambda l, i, child: enc[i * min(bs_opt, max(len(enc), 1)) ** l].ljust(ks, b"\0") + struct.pack("<Q", child),
                           head_bytes + 32)
    ctree = struct.pack("<IIIIQQ", CHROM_MAGIC, min(bs_opt, max(len(enc), 1)), ks, 8, len(enc), 0) + ctree_nodes
    # ---- full data
    payloads, bounds = [], []
    for cid, t in enumerate(chrom_tids):
        rows = np.flatnonzero(tid == t)
        for k in range(0, len(rows), S):
            r = rows[k:k + S]
            body = b"".join(struct.pack("<II", int(start[i]), int(end[i])) + value_of(dep[i], wide).tobytes() for i in r)
            payloads.append(struct.pack("<IIIIIBBH", cid, int(start[r[0]]), int(end[r[-1]]), 0, 0, 1, 0, len(r)) + body)
            bounds.append(((cid, int(start[r[0]])), (cid, int(end[r[-1]]))))

    def data_and_index(count, payloads, bounds, at):
        streams = [pack(p) for p in payloads]
        where = np.concatenate([[0], np.cumsum([len(s) for s in streams], dtype=np.int64)]).astype(np.int64).tolist()
        data = count + b"".join(streams)
        return data, _rtree(bounds, where, at + len(count), bs_opt, at + len(data))
    at = head_bytes + len(ctree)
    data_off = at
    data, index = data_and_index(struct.pack("<Q", len(payloads)), payloads, bounds, at)
    index_off = at + len(data)
    body = data + index
    at += len(body)
    # ---- zoom levels
    zooms, exact = [], []
    for k in range(Z):
        R = R0 * 4 ** k
        rec, ex = zoom_records(cov["depth"], lens, chrom_tids, R, wide)
        exact.append(ex)
        blocks = [rec[i:i + S] for i in range(0, len(rec), S)]
        zb = [((int(b["chrom"][0]), int(b["start"][0])), (int(b["chrom"][-1]), int(b["end"][-1]))) for b in blocks]
        data, index = data_and_index(struct.pack("<I", len(rec)), [b.tobytes() for b in blocks], zb, at)
        zooms.append((R, at, at + len(data)))
        body += data + index
        at += len(data) + len(index)
    ubuf = max(24 + 12 * S, 32 * S) if compress else 0
    head = struct.pack("<IHHQQQHHQQIQ", BIGWIG_MAGIC, 4, Z, head_bytes, data_off, index_off, 0, 0, 0, 64 + 24 * Z, ubuf, 0)
    head += b"".join(struct.pack("<IIQQ", R, 0, d, i) for R, d, i in zooms)
    head += struct.pack("<Qdddd", *total_summary(cov["depth"], chrom_tids, wide))
    return head + ctree + body + struct.pack("<I", BIGWIG_MAGIC), {"zoom_exact": exact}


def ulp_apart(a, b):
    """how many float32 values lie between two non-negative float32 arrays, elementwise"""
    return np.abs(np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64))

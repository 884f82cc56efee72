"""The yardstick of --quant-bam (br_assign): the tests' own restatement, in numpy and Python, of the definitions in bramble_amd.h --
placement, m, w, ZW, the draw, the rewritten record -- which the GPU tests compare the device against bit for bit.  Every
floating-point step is one np.float64 operation in the stated order."""
import struct

import numpy as np

from tests import bamio
from tests.test_quant_boot_cpu import philox4x32_10
from tests.test_quant_fld_cpu import ROW_FIRST, ROW_PAIRED, ROW_PRIMARY, ROW_SAME_TX

MODES = {"tag": 0, "sample": 1}
MAPQ_UNIQUE = {0: 255, 1: 3}   # br_row_mapq(1, long_reads)


def placements_of(meta, row_off, group_off):
    """-> (lead, per_name): lead[r] = the first record of r's placement; per_name[g] = the leaders of name g in record order.
    ValueError for a record that belongs to no placement or a PAIRED leader without its mate inside the name."""
    meta = np.asarray(meta, dtype=np.uint64)
    lead = np.full(len(meta), -1, dtype=np.int64)
    per_name = []
    for g in range(len(group_off) - 1):
        r0, r1 = int(row_off[int(group_off[g])]), int(row_off[int(group_off[g + 1])])
        mine, r = [], r0
        while r < r1:
            m = int(meta[r])
            if not m & ROW_FIRST:
                raise ValueError("record %d belongs to no placement" % r)
            mine.append(r)
            lead[r] = r
            if m & ROW_PAIRED:
                if r + 1 >= r1 or not int(meta[r + 1]) & ROW_PAIRED or int(meta[r + 1]) & ROW_FIRST:
                    raise ValueError("record %d leads a pair without a mate inside its name" % r)
                lead[r + 1] = r
                r += 1
            r += 1
        per_name.append(mine)
    return lead, per_name


def weights_of(post, cl, name_cls, row_name, tids, placements):
    """post: the posterior per label entry, class after class (posteriors_of); cl: classes_of; -> (w float64 per record: the w of
    its placement, m per record)"""
    lead, per_name = placements
    n = len(tids)
    off = np.concatenate([[0], np.cumsum([len(s) for s in cl["labels"]])])
    p = np.zeros(n, dtype=np.float64)
    for r in range(n):
        c = int(name_cls[int(row_name[r])])
        p[r] = post[int(off[c]) + cl["labels"][c].index(int(tids[r]))]
    m = np.zeros(n, dtype=np.int64)
    count = {}
    for r in range(n):
        k = (int(row_name[r]), int(tids[r]))
        count[k] = count.get(k, 0) + 1
    for r in range(n):
        m[r] = count[(int(row_name[r]), int(tids[r]))]
    w = np.zeros(n, dtype=np.float64)
    for r in range(n):
        r0 = int(lead[r])
        if r0 != r:
            continue
        v = np.float64(p[r0]) / np.float64(m[r0])
        if r0 + 1 < n and int(lead[r0 + 1]) == r0:
            v = v + np.float64(p[r0 + 1]) / np.float64(m[r0 + 1])
            w[r0 + 1] = v
        w[r0] = v
    return w, m


def uniform_of(names, seed):
    """U per name: Philox4x32-10 under the seed's two words at the counter (name & 0xffffffff, name >> 32, 0, 1)"""
    seed &= 0xffffffffffffffff
    g = np.asarray(names, dtype=np.uint64)
    if not len(g):
        return np.zeros(0, dtype=np.float64)
    out = philox4x32_10((g & np.uint64(0xffffffff), g >> np.uint64(32), np.zeros(len(g), np.uint64), np.ones(len(g), np.uint64)),
                        (seed & 0xffffffff, seed >> 32))
    u = out[0] | (out[1] << np.uint64(32))
    return (u >> np.uint64(11)).astype(np.float64) * np.float64(2.0 ** -53)


def pick_of(ws, U):
    """the draw among a name's placements of weights ws (in order) at the uniform U -> the placement's number"""
    W = np.float64(0.0)
    for v in ws:
        W = W + np.float64(v)
    target = np.float64(U) * W
    cum = np.float64(0.0)
    for j, v in enumerate(ws):
        cum = cum + np.float64(v)
        if cum > target:
            return j
    positive = [j for j, v in enumerate(ws) if v > 0]
    return positive[-1] if positive else 0


def picks_of(w, placements, seed):
    """-> the picked placement's number per name, -1 for a name without placements"""
    _, per_name = placements
    U = uniform_of(np.arange(len(per_name)), seed)
    return np.asarray([pick_of([w[r] for r in mine], U[g]) if mine else -1 for g, mine in enumerate(per_name)], dtype=np.int64)


def kept_of(w, placements, mode, seed):
    lead, per_name = placements
    if MODES[mode] == 0:
        return np.ones(len(lead), dtype=np.uint8)
    picked = [mine[j] for mine, j in zip(per_name, picks_of(w, placements, seed)) if j >= 0]
    return np.isin(lead, np.asarray(picked, dtype=np.int64)).astype(np.uint8)


def aux_entries(aux):
    """(offset, tag, type, size of the whole entry) of every entry of an aux area, walked from its start"""
    out, p = [], 0
    while p + 3 <= len(aux):
        ty = aux[p + 2:p + 3]
        if ty in b"AcC":
            n = 1
        elif ty in b"sS":
            n = 2
        elif ty in b"iIf":
            n = 4
        elif ty in b"ZH":
            n = aux.index(b"\0", p + 3) - (p + 3) + 1
        elif ty == b"B":
            sub = aux[p + 3:p + 4]
            n = 5 + {b"c": 1, b"C": 1, b"s": 2, b"S": 2}.get(sub, 4) * struct.unpack_from("<I", aux, p + 4)[0]
        else:
            raise ValueError("aux type %r" % ty)
        out.append((p, aux[p:p + 2], ty, 3 + n))
        p += 3 + n
    assert p == len(aux)
    return out


def rewrite_one(rec, zw_bits, mode, long_reads):
    """rec: [block_size][record] -> its rewritten form"""
    size = struct.unpack_from("<I", rec, 0)[0]
    assert size + 4 == len(rec)
    body = bytearray(rec[4:])
    if MODES[mode] == 1:
        f = bamio.record_fields(bytes(body))
        at = len(body) - len(f["aux"])
        entries = aux_entries(f["aux"])
        for tag in (b"NH", b"HI"):
            mine = [e for e in entries if e[1] == tag and e[2] == b"i"]
            struct.pack_into("<i", body, at + mine[-1][0] + 3, 1)
        struct.pack_into("<H", body, 14, f["flag"] & ~0x100)
        body[9] = MAPQ_UNIQUE[int(bool(long_reads))]
    return struct.pack("<I", size + 7) + bytes(body) + b"ZWf" + struct.pack("<I", int(zw_bits))


def rewrite(records, zw, kept, mode, long_reads=False):
    """records: [block_size][record] byte strings in add order; zw: float32 per record; kept: per record -> the stream (uint8)"""
    bits = np.asarray(zw, dtype=np.float32).view(np.uint32)
    out = [rewrite_one(r, bits[i], mode, long_reads) for i, r in enumerate(records) if kept[i]]
    return np.frombuffer(b"".join(out), dtype=np.uint8)


def zw_of(w):
    """float32 of every w, rounded to nearest even (numpy's conversion)"""
    return np.asarray(w, dtype=np.float64).astype(np.float32)


# ---- a hand-built table -------------------------------------------------------------------------------------------------------
HAND_N_TX = 80
HAND_LENS = np.asarray([300 + 37 * (t % 11) for t in range(HAND_N_TX)], dtype=np.int64)


def hand_built():
    """Names (each a list of (transcript, meta bits) records) for what the generated tables do not hold: a name of one record; a
    name of 130 placements over 70 transcripts (m by the wave, more than 64 labels); a name of 65 records on one transcript (32
    pairs and a single); a pair on two transcripts (SAME_TX clear); a name without rows between two names with rows; names of
    several records as the first and the last name of every add of the three-call cut (n // 3, n // 3 + 1)."""
    F, LEAD, LEAD2, MATE = ROW_FIRST, ROW_FIRST | ROW_PAIRED | ROW_SAME_TX, ROW_FIRST | ROW_PAIRED, ROW_PAIRED
    MATE1 = ROW_PAIRED | ROW_SAME_TX
    multi = [(5, LEAD | ROW_PRIMARY), (5, MATE1), (6, F), (5, F), (7, LEAD2), (8, MATE)]
    names = [[(t % HAND_N_TX, F | ROW_PRIMARY), ((t * 7 + 3) % HAND_N_TX, F)] if t % 3 else [(t % HAND_N_TX, F | ROW_PRIMARY)] for t in range(60)]
    names[0] = list(multi)
    names[-1] = [(9, F | ROW_PRIMARY), (9, F), (10, LEAD2), (11, MATE)]
    k = len(names) // 3
    names[k - 1] = list(multi)
    names[k] = [(20, LEAD2 | ROW_PRIMARY), (21, MATE)]                     # a call of this one name
    names[k + 1] = [(6, F | ROW_PRIMARY)] + list(multi[:2])
    names[3] = [(40, F | ROW_PRIMARY)]                                     # one record
    names[5] = [((3 * j) % 70, F | (ROW_PRIMARY if j == 0 else 0)) for j in range(130)]
    names[7] = [(33, m) for _ in range(32) for m in (LEAD, MATE1)] + [(33, F)]
    names[9], names[10], names[11] = [(50, F | ROW_PRIMARY)], [], [(51, F | ROW_PRIMARY), (50, F)]
    names[30] = []
    return names, HAND_LENS


def table_of(names):
    """names: lists of (tid, meta bits) -> tids, meta, row_off, group_off (one alignment a record)"""
    tids = np.asarray([t for nm in names for t, _ in nm], dtype=np.uint32)
    meta = np.asarray([m for nm in names for _, m in nm], dtype=np.uint32)
    row_off = np.concatenate([[0], np.cumsum([len(nm) for nm in names])]).astype(np.uint64)
    return tids, meta, row_off, np.arange(len(names) + 1, dtype=np.uint32)

"""--sort without a GPU: the tests' own restatement of the coordinate order (bramble_amd.h: br_sorter) and of the BAI layout
br_sorter_index writes (SAM specification 5.1.1 reg2bin / reg2bins, 5.2), which the GPU tests compare the device against; checks
of those yardsticks against values worked out by hand; the ABI without a device and the command line's usage errors."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")

MAX_END = 1 << 29
PSEUDO_BIN = 37450


# ---- the yardsticks: records are bytes from refID on (without block_size), as bamio.split_stream returns them ---------------
def sort_key(rec):
    ref, pos = struct.unpack_from("<ii", rec, 0)
    flag = struct.unpack_from("<H", rec, 14)[0]
    return ((ref & 0xffffffff) << 32) | (((pos + 1) & 0xffffffff) << 1) | ((flag >> 4) & 1)


def coordinate_order(records):
    """indices of `records` in coordinate order: a stable sort on the 64-bit key"""
    return sorted(range(len(records)), key=lambda i: sort_key(records[i]))


def ref_pos_end(rec):
    """(refID, pos, end): end = pos + the reference length of the CIGAR field (M D N = X), pos + 1 when that is 0"""
    ref, pos = struct.unpack_from("<ii", rec, 0)
    l_name, n_cig = rec[8], struct.unpack_from("<H", rec, 12)[0]
    rl = 0
    for k in range(n_cig):
        w = struct.unpack_from("<I", rec, 32 + l_name + 4 * k)[0]
        if (w & 15) in (0, 2, 3, 7, 8):
            rl += w >> 4
    return ref, pos, pos + (rl if rl else 1)


def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    bins = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        bins.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return bins


def bai_bytes(records, voffsets, n_ref):
    """The index of `records` (file order) whose begin virtual offsets are voffsets[0 .. n) and whose last record ends at
    voffsets[n]: bins ascending, consecutive records of the file in one bin merged into a chunk and nothing else, the pseudo-bin
    last, the linear index filled from the right, n_no_coor at the end."""
    assert len(voffsets) == len(records) + 1
    bins = [dict() for _ in range(n_ref)]      # bin -> [[beg, end, index of its last record]]
    lin = [dict() for _ in range(n_ref)]
    stat = [None] * n_ref                      # [first record, last record, mapped, unmapped]
    no_coor = 0
    for i, rec in enumerate(records):
        ref, pos, end = ref_pos_end(rec)
        assert ref < n_ref
        if ref < 0 or pos < 0:
            no_coor += 1
            continue
        if end > MAX_END:
            raise ValueError("end beyond 2^29")
        chunks = bins[ref].setdefault(reg2bin(pos, end), [])
        if chunks and chunks[-1][2] == i - 1:
            chunks[-1][1], chunks[-1][2] = voffsets[i + 1], i
        else:
            chunks.append([voffsets[i], voffsets[i + 1], i])
        for w in range(pos >> 14, ((end - 1) >> 14) + 1):
            lin[ref][w] = min(lin[ref].get(w, voffsets[i]), voffsets[i])
        unmapped = (struct.unpack_from("<H", rec, 14)[0] >> 2) & 1
        if stat[ref] is None:
            stat[ref] = [i, i, 0, 0]
        stat[ref][1] = i
        stat[ref][2 + unmapped] += 1
    out = bytearray(b"BAI\1" + struct.pack("<i", n_ref))
    for r in range(n_ref):
        out += struct.pack("<i", len(bins[r]) + (1 if stat[r] else 0))
        for b in sorted(bins[r]):
            out += struct.pack("<Ii", b, len(bins[r][b]))
            for beg, end, _ in bins[r][b]:
                out += struct.pack("<QQ", beg, end)
        if stat[r]:
            first, last, n_map, n_unm = stat[r]
            out += struct.pack("<IiQQQQ", PSEUDO_BIN, 2, voffsets[first], voffsets[last + 1], n_map, n_unm)
        n_intv = 1 + max(lin[r]) if lin[r] else 0
        out += struct.pack("<i", n_intv)
        vals, nxt = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            nxt = lin[r].get(w, nxt)
            vals[w] = nxt
        out += b"".join(struct.pack("<Q", v) for v in vals)
    return bytes(out + struct.pack("<Q", no_coor))


def bai_parse(bai):
    """-> ([(bins {bin: [(beg, end)]}, ioffsets)] per reference, n_no_coor)"""
    assert bai[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", bai, 4)[0]
    p, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", bai, p)[0]
        p += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", bai, p)
            p += 8
            bins[b] = [struct.unpack_from("<QQ", bai, p + 16 * k) for k in range(n_chunk)]
            p += 16 * n_chunk
        n_intv = struct.unpack_from("<i", bai, p)[0]
        p += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, bai, p))))
        p += 8 * n_intv
    assert p + 8 == len(bai)
    return refs, struct.unpack_from("<Q", bai, p)[0]


def bai_query(bai, tid, beg, end):
    """The specification's query: the chunks of reg2bins(beg, end) on `tid` that end behind the linear index's lower bound"""
    bins, ioff = bai_parse(bai)[0][tid]
    if not ioff:
        return []
    min_off = ioff[min(beg >> 14, len(ioff) - 1)]
    chunks = []
    for b in reg2bins(beg, end):
        chunks.extend(c for c in bins.get(b, []) if c[1] > min_off)
    return sorted(chunks)


# ---- the yardsticks against values worked out by hand -------------------------------------------------------------------------
def test_reg2bin_at_the_level_boundaries():
    assert reg2bin(0, 1) == 4681
    assert reg2bin(0, 16385) == 585
    assert reg2bin(0, 1 << 29) == 0
    assert reg2bin((1 << 29) - 2, (1 << 29) - 1) == 37448
    assert reg2bins(0, 1) == [0, 1, 9, 73, 585, 4681]
    assert reg2bins(16383, 16385) == [0, 1, 9, 73, 585, 4681, 4682]


def _rec(name, ref, pos, length, flag=0):
    return bamio.bam_record(name, ref, pos, [length << 4] if length else [], max(length, 1), flag=flag)


def test_coordinate_order_key():
    recs = [_rec(b"a", 1, 5, 10), _rec(b"b", -1, -1, 0, flag=4), _rec(b"c", 0, 7, 10, flag=16), _rec(b"d", 0, 7, 10), _rec(b"e", 0, 7, 10, flag=16),
            _rec(b"f", 0, 6, 10, flag=16), _rec(b"g", 0, 7, 10)]
    # reference 0 first, by position; at position 7 the forward strand (d, g) in front of the reverse one (c, e), each in the
    # order given; refID -1 last
    assert coordinate_order(recs) == [5, 3, 6, 2, 4, 0, 1]
    again = [recs[i] for i in coordinate_order(recs)]
    assert coordinate_order(again) == list(range(len(again)))
    assert ref_pos_end(recs[0]) == (1, 5, 15) and ref_pos_end(recs[1]) == (-1, -1, 0)
    spilled = bamio.bam_record(b"s", 0, 100, [20 << 4, (30 << 4) | 3, 20 << 4], 40, spill=True)
    assert ref_pos_end(spilled) == (0, 100, 170)


def test_three_record_index_by_hand():
    a = _rec(b"a", 0, 100, 50)            # [100, 150): bin 4681, window 0
    b = _rec(b"b", 0, 16380, 10)          # [16380, 16390): windows 0 and 1 -> bin 585
    c = _rec(b"c", -1, -1, 0, flag=4)     # no coordinate
    va, vb, vc, ve = 1 << 16, (1 << 16) | 100, (1 << 16) | 200, 50 << 16
    exp = b"BAI\1" + struct.pack("<i", 2)
    exp += struct.pack("<i", 3)                                            # reference 0: two bins and the pseudo-bin
    exp += struct.pack("<IiQQ", 585, 1, vb, vc)
    exp += struct.pack("<IiQQ", 4681, 1, va, vb)
    exp += struct.pack("<IiQQQQ", 37450, 2, va, vc, 2, 0)
    exp += struct.pack("<iQQ", 2, va, vb)                                  # window 0: a (and b), window 1: b
    exp += struct.pack("<ii", 0, 0)                                        # reference 1: nothing
    exp += struct.pack("<Q", 1)
    got = bai_bytes([a, b, c], [va, vb, vc, ve], 2)
    assert got == exp
    assert bai_query(got, 0, 120, 130) == [(va, vb), (vb, vc)]             # bin 585 is searched too; the reader drops b by its position
    assert bai_query(got, 0, 16384, 16385) == [(vb, vc)]                   # window 1: bin 4682 is empty, bin 585 holds b
    assert bai_query(got, 1, 0, 100) == []
    # consecutive records of one bin are one chunk; an empty window takes the next one's value
    d = _rec(b"d", 0, 110, 10)
    e = _rec(b"e", 0, 40000, 10)
    got = bai_bytes([a, d, e], [10, 20, 30, 40], 1)
    refs, no_coor = bai_parse(got)
    assert refs[0][0] == {4681: [(10, 30)], 4683: [(30, 40)], 37450: [(10, 40), (3, 0)]} and refs[0][1] == [10, 30, 30] and no_coor == 0
    with pytest.raises(ValueError):
        bai_bytes([_rec(b"x", 0, MAX_END - 5, 10)], [0, 1], 1)


# ---- ABI and usage errors -------------------------------------------------------------------------------------------------
def test_sorter_new_without_a_device():
    """BR_ERR_NO_DEVICE for a device that does not exist (every device, on a machine without one)."""
    from bramble_amd import lib
    L = lib.lib()
    L.br_sorter_new.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.br_sorter_free.argtypes = [C.c_void_p]
    h = C.c_void_p()
    assert L.br_sorter_new(4096, C.byref(h)) == -2   # BR_ERR_NO_DEVICE
    assert not h.value
    assert L.br_sorter_new(-1, C.byref(h)) == -2
    L.br_sorter_free(None)
    for name in ("br_sorter_set_param", "br_sorter_add", "br_sorter_finish", "br_sorter_next", "br_sorter_order", "br_sorter_stats",
                 "br_sorter_index", "br_ctx_last_device_bam", "br_device_bam_download"):
        assert hasattr(L, name), name
    assert L.br_sorter_finish(None, None) == -1 and L.br_sorter_index(None, 0, None, 0, 0, None, None) == -1


@pytest.mark.parametrize("extra,word", [
    (["--write-index"], b"--sort"),
    (["--sort", "--write-index", "-O", "sam"], b"--write-index"),
    (["--sort", "--write-index", "--host-deflate"], b"--write-index"),
    (["--sort", "--write-index", "--compression-level", "1"], b"--write-index"),
    (["--sort", "--devices", "0,0"], b"--sort"),
])
def test_cli_sort_usage_errors(tmp_path, extra, word):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "o.bam")
    r = subprocess.run([BIN, str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", out] + extra, capture_output=True, timeout=60)
    assert r.returncode == 2
    assert word in r.stderr and b"usage:" in r.stderr
    for p in (out, out + ".tmp-bramble", out + ".bai", out + ".bai.tmp-bramble"):
        assert not os.path.exists(p)


def test_cli_write_index_to_standard_output_is_a_usage_error(tmp_path):
    gtf = tmp_path / "g.gtf"
    gtf.write_text('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    r = subprocess.run([BIN, str(tmp_path / "missing.bam"), "-G", str(gtf), "-o", "-", "--sort", "--write-index"], capture_output=True, timeout=60)
    assert r.returncode == 2 and b"--write-index" in r.stderr and b"usage:" in r.stderr and r.stdout == b""

"""--sort on the GPU: br_sorter's order, pieces and BAI index against the tests' restatements (test_sort_cpu.py: coordinate_order,
bai_bytes, bai_query) on the oracle's projected streams and on hand-built records, and the command line with --sort and
--write-index against the run without them (both BAM readers, stdin, SAM input, --collate, bundle sizes, --lr, the host codec,
-O sam, the @HD rewrite)."""
import bisect
import os
import random
import struct

import numpy as np
import pytest

from bramble_amd import lib, synth
from oracle import oracle_binding as ob
from tests import bamio
from tests.test_gpu_collate import _cat, _coordinate_stream, _files, _inputs, _named_records, _report, _run
from tests.test_sam_cpu import records_to_sam_py
from tests.test_sort_cpu import bai_bytes, bai_query, coordinate_order, ref_pos_end, sort_key

pytestmark = pytest.mark.gpu


def _projected(mode):
    """the oracle's projected record stream of a synthetic input, and its reference count"""
    annd, recs, _ = _inputs(mode)
    stream = _cat(recs)
    roff, rlen, _, _ = lib.bam_split(stream)
    ref_map = np.arange(len(annd["refnames"]), dtype=np.int32)
    orc, _, _, _ = ob.run_bam(ob.OracleIndex(annd), ob.make_flags(**({"lr": 1} if mode == "ont" else {})), stream, roff, rlen, ref_map)
    return np.asarray(orc["bam_stream"], dtype=np.uint8), len(annd["transcripts"])


def _sorter(stream, device_add=False, pieces=1, max_bytes=0):
    s = lib.Sorter(0)
    if max_bytes:
        s.set_param("max_bytes", max_bytes)
    if not device_add:
        s.add_host(stream)
        return s
    import torch
    recs = bamio.split_stream(stream)
    for chunk in np.array_split(np.arange(len(recs)), pieces):
        if not len(chunk):
            continue
        sub = bamio.frame([recs[i] for i in chunk])
        off = lib.Sorter.row_offsets(sub).astype(np.int64)
        s.add_device(torch.from_numpy(sub.copy()).cuda(), torch.from_numpy(off).cuda())
    return s


def _drain(s, max_bytes):
    """the pieces of a finished sorter: every one whole records, within max_bytes or a single record"""
    parts = []
    for data, off in s.pieces(max_bytes):
        assert off[0] == 0 and off[-1] == data.size and len(off) >= 2
        assert data.size <= max_bytes or len(off) == 2
        p = 0
        for k in range(len(off) - 1):   # the row table is the block_size chain
            assert off[k] == p
            p += 4 + struct.unpack_from("<I", data, p)[0]
        assert p == data.size
        parts.append(data)
    return np.concatenate(parts) if parts else np.zeros(0, np.uint8)


@pytest.mark.parametrize("mode,min_ties,min_both", [("pe", 1300, 40), ("ont", 400, 140)])
def test_sorter_against_the_yardstick(mode, min_ties, min_both):
    stream, _ = _projected(mode)
    recs = bamio.split_stream(stream)
    exp = coordinate_order(recs)
    # the input has what the order is about: records in full-key ties, positions that hold both strands, and no order yet
    keys = [sort_key(r) for r in recs]
    count = {}
    for k in keys:
        count[k] = count.get(k, 0) + 1
    ties = sum(c for c in count.values() if c > 1)
    both = sum(1 for k in count if not k & 1 and (k | 1) in count)
    print("%s: %d records, %d in full-key ties, %d both-strand positions" % (mode, len(recs), ties, both))
    assert ties >= min_ties and both >= min_both and exp != list(range(len(recs)))
    want = bamio.frame([recs[i] for i in exp])
    for device_add in (False, True):
        for max_bytes in (64 << 10, 1 << 30):
            s = _sorter(stream, device_add=device_add, pieces=3)
            assert s.finish() == len(recs)
            assert list(s.order()) == exp
            got = _drain(s, max_bytes)
            assert np.array_equal(got, want), (device_add, max_bytes)
            st = s.stats()
            assert st["arena_bytes"] == stream.size and st["peak_bytes"] >= stream.size
            s.close()


def _hand(name, ref, pos, length, flag=0):
    """a record that covers [pos, pos + length) with a short read: 5M <length - 10>N 5M"""
    cig = [5 << 4, ((length - 10) << 4) | 3, 5 << 4] if length > 10 else ([length << 4] if length else [])
    return bamio.bam_record(name, ref, pos, cig, 10 if length > 10 else max(length, 1), flag=flag)


def _hand_set():
    """records on four references that reach all six bin levels, with ties, both strands, an unmapped record that has a position,
    records without a reference and positions up to 2^29 - 2, in no order"""
    recs = []
    for lvl, edge in enumerate((1 << 26, 1 << 23, 1 << 20, 1 << 17, 1 << 14)):   # a record across each level's boundary
        for k in range(3):
            recs.append(_hand(b"x%d_%d" % (lvl, k), 0, 3 * edge - 40 - k, 100 + k, flag=16 * (k & 1)))
    for k in range(40):   # level 5, some of them at one position on both strands
        recs.append(_hand(b"s%d" % k, 0, 1000 + 7 * (k // 4), 50, flag=16 * (k & 1)))
    recs.append(_hand(b"far", 0, (1 << 29) - 2, 1))
    recs.append(_hand(b"far2", 0, (1 << 29) - 200, 200))
    recs.append(_hand(b"um", 1, 500, 0, flag=4))        # flag 0x4 with a position: in a bin, counted as unmapped
    recs.append(_hand(b"m1", 1, 500, 30))
    recs.append(_hand(b"w", 1, 70000, 60000))           # four windows, windows before it empty
    for k in range(5):
        recs.append(_hand(b"n%d" % k, -1, -1, 0, flag=4))
    recs.append(_hand(b"neg", 3, -1, 0))                # a reference but no position: no coordinate
    for k in range(20):
        recs.append(_hand(b"t%d" % k, 3, 200000 - 9000 * k, 12000, flag=16 * (k % 3 == 0)))
    random.Random(11).shuffle(recs)
    return recs


def test_sorter_hand_built_records():
    recs = _hand_set()
    exp = coordinate_order(recs)
    by_ref = [struct.unpack_from("<i", recs[i], 0)[0] for i in exp]
    assert by_ref[-5:] == [-1] * 5 and -1 not in by_ref[:-5]                       # refID -1 sorts last
    assert max(ref_pos_end(r)[1] for r in recs) == (1 << 29) - 2
    for order in ("given", "sorted", "reversed"):
        inp = recs if order == "given" else [recs[i] for i in exp] if order == "sorted" else [recs[i] for i in reversed(exp)]
        want = coordinate_order(inp)
        if order == "sorted":
            assert want == list(range(len(inp)))
        s = _sorter(bamio.frame(inp), device_add=(order == "reversed"), pieces=2)
        assert s.finish() == len(inp) and list(s.order()) == want
        assert np.array_equal(_drain(s, 300), bamio.frame([inp[i] for i in want]))
        s.close()
    # empty
    s = lib.Sorter(0)
    assert s.finish() == 0 and s.next_records(1 << 20).n_rows == 0 and len(s.order()) == 0
    assert s.index(2, [], 28) == bai_bytes([], [28 << 16], 2)
    s.close()
    # the arena cap, and add after finish
    stream = bamio.frame(recs)
    off = lib.Sorter.row_offsets(stream)
    db = lib.BrDeviceBam(stream.ctypes.data, stream.size, off.ctypes.data, len(off) - 1)
    s = lib.Sorter(0)
    s.set_param("max_bytes", stream.size // 2)
    assert s.add_records(db, False) == -5   # BR_ERR_CAPACITY
    s.close()                               # (still to be freed)
    s = _sorter(stream)
    s.finish()
    assert s.add_records(db, False) == -1   # BR_ERR_INVALID_ARG after finish
    s.close()


def _blocks_of(bgzf, base):
    """[(coffset, uoffset)] of the blocks of a BGZF byte string that starts at file offset `base`, and its EOF block's offset"""
    p, u, out = 0, 0, []
    while p < len(bgzf):
        bsize = struct.unpack_from("<H", bgzf, p + 16)[0] + 1
        isize = struct.unpack_from("<I", bgzf, p + bsize - 4)[0]
        out.append((base + p, u))
        u += isize
        p += bsize
    assert out[-1][1] == u and len(bgzf) - 28 == out[-1][0] - base   # the last one is the empty EOF block
    return out[:-1], out[-1][0]


def _voffsets(recs, blocks, eof):
    """begin virtual offset of every record of a framed stream, and the end of the last one"""
    starts = [b[1] for b in blocks]
    vo, u = [], 0
    for r in recs:
        k = bisect.bisect_right(starts, u) - 1
        vo.append(blocks[k][0] << 16 | (u - blocks[k][1]))
        u += 4 + len(r)
    return vo + [eof << 16]


def _check_queries(bai, recs, vo, n_ref, seed):
    """200 random regions: the records inside the query's chunks that overlap the region are exactly those that overlap it"""
    rng = random.Random(seed)
    spans = [ref_pos_end(r) for r in recs]
    placed = [i for i, (ref, pos, _) in enumerate(spans) if ref >= 0 and pos >= 0]
    hits = 0
    for _ in range(200):
        ref, pos, end = spans[rng.choice(placed)]
        tid = ref if rng.random() < 0.9 else rng.randrange(n_ref)
        beg = max(0, pos + rng.choice((0, rng.randrange(-60, 60), rng.randrange(-40000, 40000))))
        qend = min(1 << 29, beg + rng.choice((1, 50, 3000, 20000, 1 << 22)))
        brute = [i for i in placed if spans[i][0] == tid and spans[i][1] < qend and spans[i][2] > beg]
        got = []
        for cb, ce in bai_query(bai, tid, beg, qend):
            for i in range(bisect.bisect_left(vo, cb), bisect.bisect_left(vo, ce)):   # (virtual offsets ascend in file order)
                if i < len(recs) and spans[i][0] == tid and spans[i][1] >= 0 and spans[i][1] < qend and spans[i][2] > beg:
                    got.append(i)
        assert sorted(set(got)) == brute, (tid, beg, qend)
        hits += len(brute)
    assert hits >= 50   # (a third of the regions start at a record: most of those on its reference find it)


@pytest.mark.parametrize("which", ["pe", "hand"])
def test_index_at_the_abi(which):
    if which == "pe":
        stream, n_ref = _projected("pe")
        n_ref += 3   # references behind the last record
    else:
        stream, n_ref = bamio.frame(_hand_set()), 5
    s = _sorter(stream)
    s.finish()
    sorted_stream = _drain(s, 1 << 30)
    recs = bamio.split_stream(sorted_stream)
    assert [recs[i] for i in coordinate_order(recs)] == recs
    if which == "hand":
        levels = {0: 0, 1: 1, 9: 2, 73: 3, 585: 4, 4681: 5}
        from tests.test_sort_cpu import reg2bin
        seen = set()
        for r in recs:
            ref, pos, end = ref_pos_end(r)
            if ref >= 0 and pos >= 0:
                seen.add(max(l for f, l in levels.items() if reg2bin(pos, end) >= f))
        assert seen == {0, 1, 2, 3, 4, 5}
    for block, base in ((4096, 1234), (0xff00, 77)):
        blocks, eof = _blocks_of(bamio.bgzf_compress(sorted_stream.tobytes(), block=block, level=1), base)
        vo = _voffsets(recs, blocks, eof)
        want = bai_bytes(recs, vo, n_ref)
        got = s.index(n_ref, blocks, eof)
        assert got == want, (which, block)
        _check_queries(got, recs, vo, n_ref, seed=block)
    s.close()


# more records than one launch of the prefix sums takes (four tiles of 2048): the sorted stream's offset table, the index's
# bin and chunk heads and the radix counts (at 70 000) go through the three-launch scan.  "by_ref": fed grouped by reference,
# so every block of 256 records is uniform in the key's reference digit (and in most of its bin digits) while the blocks
# differ: the digits the radix sorts skip must come from the OR / AND over ALL blocks
@pytest.mark.parametrize("feed", ["shuffled", "by_ref"])
@pytest.mark.parametrize("n", [8193, 70000])
def test_sorter_sizes_beyond_one_scan_launch(n, feed):
    recs = [r[4:] for r in _named_records(n)]
    if feed == "by_ref":
        recs.sort(key=lambda r: -struct.unpack_from("<i", r, 0)[0])   # (stable: positions stay shuffled; references descend)
        assert len(set(struct.unpack_from("<i", r, 0)[0] for r in recs[-256:])) == 1
    exp = coordinate_order(recs)
    assert exp != list(range(n))
    s = _sorter(bamio.frame(recs))
    assert s.finish() == n
    assert list(s.order()) == exp
    want = [recs[i] for i in exp]
    sorted_stream = _drain(s, 1 << 30)
    assert np.array_equal(sorted_stream, bamio.frame(want))
    blocks, eof = _blocks_of(bamio.bgzf_compress(sorted_stream.tobytes(), block=0xff00, level=1), 77)
    vo = _voffsets(want, blocks, eof)
    assert s.index(3, blocks, eof) == bai_bytes(want, vo, 3)
    s.close()


def test_index_refuses_an_end_beyond_the_bins():
    recs = [_hand(b"a", 0, 100, 50), _hand(b"b", 0, (1 << 29) - 5, 10)]
    stream = bamio.frame(recs)
    s = _sorter(stream)
    s.finish()
    blocks, eof = _blocks_of(bamio.bgzf_compress(stream.tobytes()), 0)
    with pytest.raises(lib.BrambleError, match=r"\(-6\)"):   # BR_ERR_UNSUPPORTED
        s.index(1, blocks, eof)
    s.close()


# ---- command line -----------------------------------------------------------------------------------------------------------
def _lines(t):
    """header lines but @HD and bramble's own @PG"""
    return [l for l in t.split("\n") if not l.startswith("@PG\tID:bramble") and not l.startswith("@HD")]


def _pair(tmp_path, tag, args, extra, stdin=None):
    """the run with and without --sort: sorted output == coordinate_order of the unsorted one, headers and reports equal"""
    a, b = str(tmp_path / ("%s_plain.bam" % tag)), str(tmp_path / ("%s_sorted.bam" % tag))
    ra = _run(args + extra, a, stdin=stdin)
    rb = _run(args + extra + ["--sort"], b, stdin=stdin)
    ta, refs_a, sa = bamio.read_bam(a)
    tb, refs_b, sb = bamio.read_bam(b)
    recs = bamio.split_stream(sa)
    assert len(recs) > 1000, tag
    assert np.array_equal(sb, bamio.frame([recs[i] for i in coordinate_order(recs)])), tag
    assert _lines(ta) == _lines(tb) and refs_a == refs_b, tag
    assert tb.split("\n")[0].startswith("@HD\t") and "SO:coordinate" in tb.split("\n")[0].split("\t"), tag
    assert _report(ra) == _report(rb) and len(_report(ra)) == 5, tag
    assert not os.path.exists(b + ".tmp-bramble")
    return tb, sb, refs_b


def test_cli_sort_inputs_and_codecs(tmp_path):
    annd, recs, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, hdr = _files(tmp_path, annd, stream, "in")
    in_sam = str(tmp_path / "in.sam")
    open(in_sam, "wb").write(hdr.encode() + synth.records_to_sam(stream, annd["refnames"]))
    sorted_bam, _ = _files(tmp_path, annd, _coordinate_stream(stream), "coord")
    base = ["-G", gtf]
    runs = {
        "device": ([in_bam, "--device-reader"], None),
        "host": ([in_bam, "--host-reader"], None),
        "stdin": (["-"], open(in_bam, "rb").read()),
        "sam": ([in_sam], None),
        "collate": ([sorted_bam, "--collate"], None),
        "tiny": ([in_bam, "--bundle-size", "3"], None),
        "small": ([in_bam, "--bundle-size", "2500"], None),
        "level1": ([in_bam, "--compression-level", "1"], None),
        "hostz": ([in_bam, "--host-deflate"], None),
    }
    for tag, (args, stdin) in runs.items():
        tb, _, _ = _pair(tmp_path, tag, args, base, stdin=stdin)
        assert tb.split("\n")[0] == "@HD\tVN:1.6\tSO:coordinate", tag   # (the input's @HD says SO:coordinate already)


def test_cli_sort_long_reads(tmp_path):
    annd, _, stream = _inputs("ont")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "ont")
    _pair(tmp_path, "lr", [in_bam, "--lr"], ["-G", gtf])


def test_cli_sort_sam_output(tmp_path):
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    o_bam, o_sam = str(tmp_path / "s.bam"), str(tmp_path / "s.sam")
    _run([in_bam, "-G", gtf, "--sort"], o_bam)
    _run([in_bam, "-G", gtf, "--sort", "-O", "sam"], o_sam)
    t, refs, s = bamio.read_bam(o_bam)
    sam = open(o_sam, "rb").read()
    n_hdr = sam.index(b"\n", sam.index(b"@CO\tGenerated")) + 1
    hdr_lines = sam[:n_hdr].decode().split("\n")
    assert hdr_lines[0] == "@HD\tVN:1.6\tSO:coordinate" and _lines(sam[:n_hdr].decode()) == _lines(t)
    assert sam[n_hdr:] == records_to_sam_py(s, [n for n, _ in refs])


@pytest.mark.parametrize("hd,want", [
    ("@HD\tVN:1.6\tSO:unsorted\tGO:query\n", "@HD\tVN:1.6\tSO:coordinate"),
    ("", "@HD\tVN:1.6\tSO:coordinate"),
    ("@HD\tVN:1.5\n", "@HD\tVN:1.5\tSO:coordinate"),
])
def test_cli_sort_rewrites_the_hd_line(tmp_path, hd, want):
    annd, _, stream = _inputs("ont")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    refs = [(n, 10 ** 7) for n in annd["refnames"]]
    hdr = hd + "@PG\tID:aligner\tPN:aligner\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    in_bam = str(tmp_path / "in.bam")
    bamio.write_bam(in_bam, hdr, refs, stream.tobytes(), block=40000)
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    _run([in_bam, "-G", gtf, "--lr"], a)
    _run([in_bam, "-G", gtf, "--lr", "--sort"], b)
    ta, tb = bamio.read_bam(a)[0], bamio.read_bam(b)[0]
    assert tb.split("\n")[0] == want and tb.count("@HD") == 1
    assert (ta.split("\n")[0] == hd.rstrip("\n")) if hd else not ta.startswith("@HD")   # without --sort: what it is today
    assert _lines(ta) == _lines(tb)


def test_cli_write_index(tmp_path):
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    in_bam, _ = _files(tmp_path, annd, stream, "in")
    for tag, extra in (("one", []), ("bundles", ["--bundle-size", "2500"])):
        out = str(tmp_path / ("%s.bam" % tag))
        _run([in_bam, "-G", gtf, "--sort", "--write-index"] + extra, out)
        t, refs, s = bamio.read_bam(out)
        recs = bamio.split_stream(s)
        assert len(recs) > 1000 and [recs[i] for i in coordinate_order(recs)] == recs
        # the file's own blocks: the header's first, then those of the record section
        import gzip
        raw = open(out, "rb").read()
        sizes = bamio.bgzf_block_sizes(out)
        p, u, table = 0, 0, []
        for bs in sizes:
            table.append((p, u))
            u += struct.unpack_from("<I", raw, p + bs - 4)[0]
            p += bs
        n_header = len(gzip.decompress(raw)) - s.size
        first = next(k for k, (_, uo) in enumerate(table) if uo == n_header)   # the record section starts a block
        blocks = [(co, uo - n_header) for co, uo in table[first:-1]]
        eof = table[-1][0]
        assert sizes[-1] == 28 and eof == len(raw) - 28
        want = bai_bytes(recs, _voffsets(recs, blocks, eof), len(refs))
        assert open(out + ".bai", "rb").read() == want, tag
        assert not os.path.exists(out + ".tmp-bramble") and not os.path.exists(out + ".bai.tmp-bramble")
    # a failed run leaves neither file
    out = str(tmp_path / "none.bam")
    r = _run([in_bam, "-G", str(tmp_path / "missing.gtf"), "--sort", "--write-index"], out, ok=False)
    assert r.returncode not in (0, 2)
    for p in (out, out + ".bai", out + ".tmp-bramble", out + ".bai.tmp-bramble"):
        assert not os.path.exists(p)


def test_sorter_refuses_what_is_no_stream():
    """a device row table that descends, and a pos that is no BAM position"""
    import torch
    recs = [_hand(b"a", 0, 100, 50), _hand(b"b", 0, 300, 50), _hand(b"c", 1, 5, 20)]
    stream = bamio.frame(recs)
    off = lib.Sorter.row_offsets(stream).astype(np.int64)
    bad = off.copy()
    bad[1], bad[2] = off[2], off[1]   # the ends are right, the inside descends
    s = lib.Sorter(0)
    d_data, d_bad, d_off = torch.from_numpy(stream.copy()).cuda(), torch.from_numpy(bad).cuda(), torch.from_numpy(off).cuda()
    db = lib.BrDeviceBam(d_data.data_ptr(), stream.size, d_bad.data_ptr(), len(recs))
    torch.cuda.synchronize()
    assert s.add_records(db, True) == -1   # BR_ERR_INVALID_ARG, nothing added
    s.add_device(d_data, d_off)
    assert s.finish() == len(recs) and list(s.order()) == [0, 1, 2]
    s.close()
    for pos in (-2, -(1 << 31), (1 << 31) - 1):
        s = _sorter(bamio.frame(recs + [_hand(b"x", 1, pos, 0)]))
        with pytest.raises(lib.BrambleError, match=r"\(-1\)"):
            s.finish()
        assert s.stats()["peak_bytes"] > 0
        s.close()
    s = _sorter(bamio.frame(recs + [_hand(b"x", 1, (1 << 31) - 2, 0)]))   # the largest position there is
    assert s.finish() == 4 and list(s.order()) == [0, 1, 2, 3]
    s.close()


def test_resident_projection_feeds_the_sorter():
    """BR_OUT_RESIDENT leaves the projected records of br_project_bam_resident in HBM (counters as ever), a sorter takes them from
    there, and br_device_bam_download brings a sorted piece home as records and as BGZF blocks"""
    import gzip
    from tests.test_gpu_collate import _collate
    annd, recs, _ = _inputs("pe")
    ref_map = np.arange(len(annd["refnames"]), dtype=np.int32)
    c = _collate(_cat(recs))
    c.finish()
    b = c.next_records(10 ** 9)
    idx = lib.Index(annd, device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config()
    plain, cnt = ctx.project_bam_resident(cfg, b, ref_map)
    db, cnt2 = ctx.project_bam_resident_kept(cfg, b, ref_map)
    assert cnt2 == cnt and db.n_bytes == plain.size and db.n_rows == cnt["n_rows"] > 1000
    s = lib.Sorter(0)
    s.add_device(db, None)
    rows = bamio.split_stream(plain)
    assert s.finish() == len(rows)
    want = bamio.frame([rows[i] for i in coordinate_order(rows)])
    piece = s.next_records(1 << 30)
    assert np.array_equal(ctx.device_bam_download(piece, 0), want)
    z = ctx.device_bam_download(piece, 1)
    assert gzip.decompress(z.tobytes() + bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")) == want.tobytes()
    s.close()
    ctx.close()
    idx.close()
    c.close()

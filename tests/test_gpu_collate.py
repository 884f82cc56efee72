"""--collate on the GPU: br_collator's order and bundles against the tests' restatement of the collation (test_collate_cpu.py),
with colliding hashes on purpose, the capacity cap, the projection of its bundles against the oracle, and the command line
with --collate against the run without it on the collated input (device reader, host reader, BAM on stdin, SAM)."""
import functools
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from bramble_amd import lib, synth
from oracle import oracle_binding as ob
from tests import bamio
from tests.test_collate_cpu import _rec, collate_order, coordinate_sorted, mapped_records, read_name
from tests.test_gpu_bam_bundle import framed_stream
from tests.test_sam_cpu import encode_sam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")


def _cat(recs):
    return np.frombuffer(b"".join(recs), dtype=np.uint8)


def _split_all(stream):
    data, out, p = bytes(stream), [], 0
    while p < len(data):
        n = struct.unpack_from("<I", data, p)[0]
        out.append(data[p:p + 4 + n])
        p += 4 + n
    return out


def _inputs(mode):
    """(annotation dict, mapped records of a collated synthetic stream, the stream with unmapped records in it)"""
    if mode == "pe":
        ann = synth.Annotation("G", n_genes=500, n_refs=3)
        b = ann.reads(2500, "pe", with_records=1, xs_tag=True)
    else:
        ann = synth.Annotation("G", n_genes=300, n_refs=2)
        b = ann.reads(800, "ont", with_records=1)
    stream = framed_stream(b, unmapped_every=23)
    if mode == "pe":   # one read with 13 alignments: a group larger than the small bundles below
        recs = _split_all(stream)
        k = next(i for i, r in enumerate(recs) if r in set(mapped_records(stream)))
        stream = _cat(recs[:k + 1] + [recs[k]] * 12 + recs[k + 1:])
    return ann.as_dict(), mapped_records(stream), stream


def _permuted(recs, how):
    if how == "coordinate":
        return coordinate_sorted(recs)
    if how == "shuffled":
        r = list(recs)
        random.Random(7).shuffle(r)
        return r
    return list(reversed(recs))


def _collate(stream, hash_bits=64, device_add=False, pieces=1):
    """a Collator holding the mapped records of `stream`: added from host memory in one call, or from HBM in `pieces` calls"""
    c = lib.Collator(0)
    if hash_bits != 64:
        c.set_param("hash_bits", hash_bits)
    if not device_add:
        c.add_host(stream)
        return c
    import torch
    recs = mapped_records(stream)
    for chunk in np.array_split(np.arange(len(recs)), pieces):
        if not len(chunk):
            continue
        sub = _cat([recs[i] for i in chunk])
        off, ln, _, _ = lib.bam_split(sub)
        c.add_device(torch.from_numpy(sub.copy()).cuda(), torch.from_numpy(off.astype(np.int64)).cuda(),
                     torch.from_numpy(ln.astype(np.int32)).cuda())
    return c


@pytest.mark.parametrize("mode", ["pe", "ont"])
@pytest.mark.parametrize("how", ["coordinate", "shuffled", "reversed"])
def test_collator_order_and_bundles(mode, how):
    _, recs, _ = _inputs(mode)
    recs = _permuted(recs, how)
    exp = collate_order(recs)
    stream = _cat(recs)
    for device_add in (False, True):
        c = _collate(stream, device_add=device_add, pieces=3)
        n, g = c.finish()
        assert n == len(recs) and g == len(set(read_name(r) for r in recs))
        assert list(c.order()) == exp
        got = np.concatenate(list(c.bundles(1000)))
        assert np.array_equal(got, _cat([recs[i] for i in exp]))
        c.close()


@pytest.mark.parametrize("bits", [0, 4, 12])
def test_collator_hash_collisions_change_nothing(bits):
    _, recs, _ = _inputs("pe")
    recs = _permuted(recs, "coordinate")
    c = _collate(_cat(recs), hash_bits=bits)
    c.finish()
    assert list(c.order()) == collate_order(recs)
    c.close()


@functools.lru_cache(maxsize=None)
def _named_records(n):
    """n minimal mapped records ([block_size][record]) whose names repeat so that the groups have 1 to 3 members, in an order
    shuffled by a fixed seed"""
    recs, g = [], 0
    while len(recs) < n:
        for _ in range(min(1 + g % 3, n - len(recs))):
            recs.append(_rec(b"q%d" % g, 100 + 37 * len(recs) % 90001, ref=len(recs) % 3, flag=16 * (len(recs) % 2)))
        g += 1
    random.Random(5).shuffle(recs)
    return tuple(recs)


# The prefix sums of the collation run over n + 1 items and, in the radix sort, over 256 counts a tile of records.  These
# sizes put n + 1 on either side of a scan tile (2048) and of the four tiles one launch takes (8192); at 70 000 the radix
# counts (256 x 35 tiles = 8960) take the three-launch scan too.
@pytest.mark.parametrize("n", [1, 2047, 2048, 2049, 8191, 8192, 8193, 70000])
def test_collator_sizes_around_the_scan_tiles(n):
    recs = list(_named_records(n))
    exp = collate_order(recs)
    groups = len(set(read_name(r) for r in recs))
    stream = _cat(recs)
    for bits in (64, 4):
        c = _collate(stream, hash_bits=bits)
        assert tuple(c.finish()) == (n, groups)
        assert list(c.order()) == exp, bits
        c.close()


def test_collator_bundles_hold_whole_groups():
    _, recs, _ = _inputs("pe")
    recs = _permuted(recs, "shuffled")
    exp = _cat([recs[i] for i in collate_order(recs)])
    sizes = {}
    for r in recs:
        sizes[read_name(r)] = sizes.get(read_name(r), 0) + 1
    assert max(sizes.values()) > 7
    for m in (1, 7, 10000):
        c = _collate(_cat(recs))
        c.finish()
        parts = list(c.bundles(m))
        for k, p in enumerate(parts):
            names = [read_name(r) for r in mapped_records(p)]
            last = len(names) - 1
            while last > 0 and names[last - 1] == names[-1]:
                last -= 1
            assert last < m   # the bundle's last group starts in front of the limit (a larger group comes alone)
            assert len(names) >= m or k == len(parts) - 1
        for a, b in zip(parts, parts[1:]):
            assert read_name(mapped_records(a)[-1]) != read_name(mapped_records(b)[0])
        assert np.array_equal(np.concatenate(parts), exp)
        c.close()
    # empty, and a single record
    c = lib.Collator(0)
    assert c.finish() == (0, 0) and list(c.bundles(5)) == [] and len(c.order()) == 0
    c.close()
    c = _collate(_cat(recs[:1]))
    assert c.finish() == (1, 1) and list(c.order()) == [0]
    assert np.array_equal(np.concatenate(list(c.bundles(5))), _cat(recs[:1]))
    c.close()


def test_collator_capacity_and_add_after_finish():
    _, recs, _ = _inputs("pe")
    stream = _cat(recs)
    c = lib.Collator(0)
    c.set_param("max_bytes", stream.size // 2)
    off, ln, _, _ = lib.bam_split(stream)
    recs_s = lib.BrDeviceRecords(stream.ctypes.data, off.ctypes.data, len(off), ln.ctypes.data)
    assert c.add_records(recs_s, False) == -5   # BR_ERR_CAPACITY
    c.close()
    c = _collate(stream)
    c.finish()
    assert c.add_records(recs_s, False) == -1   # BR_ERR_INVALID_ARG after finish
    c.close()


@pytest.mark.parametrize("mode,flags", [("pe", {}), ("ont", {"lr": 1})])
def test_collator_bundles_project_like_the_oracle(mode, flags):
    annd, recs, _ = _inputs(mode)
    recs = _permuted(recs, "coordinate")
    collated = _cat([recs[i] for i in collate_order(recs)])
    ref_map = np.arange(len(annd["refnames"]), dtype=np.int32)
    c = _collate(_cat(recs), device_add=True, pieces=2)
    c.finish()
    idx = lib.Index(annd, device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config(**flags)
    streams, tot = [], {}
    while True:
        b = c.next_records(700)
        if b.n_aln == 0:
            break
        s, cnt = ctx.project_bam_resident(cfg, b, ref_map)
        streams.append(s)
        for k, v in cnt.items():
            tot[k] = tot.get(k, 0) + v
    ctx.close()
    idx.close()
    c.close()
    roff, rlen, _, _ = lib.bam_split(collated)
    orc, _, _, _ = ob.run_bam(ob.OracleIndex(annd), ob.make_flags(**flags), collated, roff, rlen, ref_map)
    assert np.array_equal(np.concatenate(streams), orc["bam_stream"])
    for k in ("total_complete", "total_unique", "dropped_reads", "total_processed"):
        assert tot[k] == orc[k], k


# ---- command line ---------------------------------------------------------------------------------------------------------
HDR = "@HD\tVN:1.6\tSO:coordinate\n@PG\tID:aligner\tPN:aligner\n"


def _files(tmp_path, annd, stream, tag):
    names = annd["refnames"]
    refs = [(n, 10 ** 7) for n in names]
    hdr = HDR + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    bam = str(tmp_path / ("%s.bam" % tag))
    bamio.write_bam(bam, hdr, refs, stream.tobytes(), block=40000)
    return bam, hdr


def _run(args, out, stdin=None, ok=True):
    r = subprocess.run([BIN] + args + ["-o", out], input=stdin, capture_output=True, timeout=600)
    if ok:
        assert r.returncode == 0, r.stderr.decode() + r.stdout.decode()
    return r


def _report(r):
    return [l for l in r.stdout.decode().split("\n") if l.startswith("# ")]


def _strip(t):
    return [l for l in t.split("\n") if not l.startswith("@PG\tID:bramble")]


def _coordinate_stream(stream):
    """the stream's records (unmapped ones included) sorted by (refID, pos), as a coordinate-sorted file holds them"""
    return _cat(coordinate_sorted(_split_all(stream)))


def _reference(tmp_path, annd, stream, extra, tag):
    """the run without the flag on the tests' collation of `stream`'s mapped records: (header, refs, records, report)"""
    recs = mapped_records(stream)
    bam, _ = _files(tmp_path, annd, _cat([recs[i] for i in collate_order(recs)]), "collated_" + tag)
    o = str(tmp_path / ("o_ref_%s.bam" % tag))
    r = _run([bam] + extra, o)
    t, refs, s = bamio.read_bam(o)
    assert len(s) > 100000
    return t, refs, s, _report(r)


def test_cli_collate_coordinate_sorted(tmp_path):
    annd, recs, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    extra = ["-G", gtf, "--compression-level", "1"]
    sorted_stream = _coordinate_stream(stream)
    in_bam, hdr = _files(tmp_path, annd, sorted_stream, "sorted")
    sorted_sam = str(tmp_path / "sorted.sam")
    names = annd["refnames"]
    text = synth.records_to_sam(sorted_stream, names)
    open(sorted_sam, "wb").write(hdr.encode() + text)
    _, _, sam_every = encode_sam(text, names)   # the SAM lines as htslib stores them: the reference of the SAM run
    ref = {"bam": _reference(tmp_path, annd, sorted_stream, extra, "bam"), "sam": _reference(tmp_path, annd, sam_every, extra, "sam")}
    # the sorted input holds the unmapped records the collated one lacks: the report differs in those two lines only
    n_unm = len(_split_all(sorted_stream)) - len(recs)
    assert n_unm > 0
    runs = {
        "device": [in_bam, "--collate", "--device-reader"],
        "host": [in_bam, "--collate", "--host-reader"],
        "stdin": ["-", "--collate"],
        "sam": [sorted_sam, "--collate"],
        "small": [in_bam, "--collate", "--bundle-size", "2500"],
        "tiny": [in_bam, "--collate", "--bundle-size", "3"],   # (the read with 13 alignments: a group larger than the bundle)
    }
    for tag, args in runs.items():
        t0, refs0, s0, rep0 = ref["sam" if tag == "sam" else "bam"]
        o = str(tmp_path / ("o_%s.bam" % tag))
        r = _run(args + extra, o, stdin=open(in_bam, "rb").read() if tag == "stdin" else None)
        t, refs, s = bamio.read_bam(o)
        assert _strip(t) == _strip(t0) and refs == refs0, tag
        assert np.array_equal(s, s0), tag
        rep = _report(r)
        assert rep[0] == "# input alignments:   %d" % (len(recs) + n_unm) and rep[1] == "# unmapped reads:     %d" % n_unm, tag
        assert rep[2:] == rep0[2:] and len(rep) == 5, tag
        assert any(l.startswith("[bramble] collated %d records" % len(recs)) for l in r.stdout.decode().split("\n")), tag


def test_cli_collate_on_collated_input_changes_nothing(tmp_path):
    annd, _, stream = _inputs("pe")
    gtf = str(tmp_path / "g.gtf")
    bamio.write_gtf(gtf, annd)
    bam, _ = _files(tmp_path, annd, stream, "in")
    extra = ["-G", gtf, "--compression-level", "1"]
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    ra, rb = _run([bam] + extra, a), _run([bam, "--collate"] + extra, b)
    ta, _, sa = bamio.read_bam(a)
    tb, _, sb = bamio.read_bam(b)
    assert _strip(ta) == _strip(tb) and np.array_equal(sa, sb) and _report(ra) == _report(rb) and len(_report(ra)) == 5


def test_cli_collate_errors(tmp_path):
    gtf = str(tmp_path / "g.gtf")
    open(gtf, "w").write('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    out = str(tmp_path / "out.bam")
    header = "@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:5000\n"
    good = "r%d\t0\tchr1\t%d\t60\t4M\t*\t0\t0\tACGT\tIIII\n"
    body = "".join(good % (k % 3, 400 - k) for k in range(5)) + "r9\t0\tchr1\t100\t60\t4Q\t*\t0\t0\tACGT\tIIII\n" + good % (1, 7)
    sam = str(tmp_path / "bad.sam")
    open(sam, "w").write(header + body)
    r = _run([sam, "-G", gtf, "--collate"], out, ok=False)
    assert r.returncode != 0
    assert ("bad.sam:%d: " % (header.count("\n") + 6)) in r.stderr.decode() and "CIGAR" in r.stderr.decode(), r.stderr.decode()
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp-bramble")
    r = _run([sam, "-G", gtf, "--collate", "--devices", "0,0"], out, ok=False)
    assert r.returncode == 2 and b"--collate" in r.stderr
    assert not os.path.exists(out)

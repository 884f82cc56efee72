"""SAM text out on the GPU: br_sam_format_device against the host formatters (records_to_sam_py, and synth.records_to_sam
for the glibc %g of floats), the bundle entry points with BR_OUT_SAM_TEXT, and `bramble -O sam` against the BAM of the same
run.  Records are assembled from the specification (tests/bamio.py)."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from bramble_amd import lib, synth
from tests import bamio
from tests.test_cg_tag_cpu import ANN, long_cigar
from tests.test_gpu_bam_bundle import framed_stream
from tests.test_sam_cpu import encode_sam, records_to_sam_py

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")
NAMES = ["chr1", "ENST00000456328.2_a_longer_transcript_name", "t3"]


def cg_restore(line, rec):
    """bam_tag2cigar on the text of one record (the rule of csrc/bam_cg.h): a mapped record whose CIGAR is <l_seq>S<ref_len>N
    and whose first CG tag is B,I / B,i with at least n_cigar entries prints those entries as its CIGAR and loses the tag."""
    f = bamio.record_fields(rec)
    cig = f["cigar"]
    if not cig or f["ref_id"] < 0 or f["pos"] < 0 or (cig[0] & 0xF) != 4 or (cig[0] >> 4) != f["l_seq"]:
        return line
    fields = line.rstrip(b"\n").split(b"\t")
    for k in range(11, len(fields)):
        if fields[k].startswith(b"CG:"):
            if not (fields[k].startswith(b"CG:B:I,") or fields[k].startswith(b"CG:B:i,")):
                return line
            ops = [int(v) for v in fields[k][7:].split(b",")]
            if len(ops) < len(cig) or len(ops) >= 1 << 29:
                return line
            fields[5] = b"".join(b"%d%s" % (w >> 4, b"MIDNSHP=XB"[min(w & 15, 9):min(w & 15, 9) + 1]) for w in ops)
            del fields[k]
            return b"\t".join(fields) + b"\n"
    return line


def records_to_sam_cg(stream, names):
    """records_to_sam_py, extended with the restore of a spilled CIGAR"""
    return b"".join(cg_restore(records_to_sam_py(bamio.frame([r]), names), r) for r in bamio.split_stream(stream))


def row_offsets(stream):
    off, p, data = [], 0, bytes(stream)
    while p < len(data):
        off.append(p)
        p += 4 + struct.unpack_from("<I", data, p)[0]
    return np.array(off, dtype=np.int64)


@pytest.fixture(scope="module")
def ctx():
    idx = lib.Index(ANN, device=0)
    c = lib.Context(idx)
    c.set_sam_refs(NAMES)
    yield c
    c.close()
    idx.close()


def fmt(ctx, stream):
    import torch
    data = torch.from_numpy(np.ascontiguousarray(stream, dtype=np.uint8).copy()).to("cuda:0")
    off = torch.from_numpy(row_offsets(stream)).to("cuda:0")
    return bytes(ctx.sam_format_device(data, off).cpu().numpy())


def raw_rc(ctx, stream):
    """the return code of br_sam_format_device on a stream"""
    import torch
    data = torch.from_numpy(np.ascontiguousarray(stream, dtype=np.uint8).copy()).to("cuda:0")
    off = torch.from_numpy(row_offsets(stream)).to("cuda:0")
    db = lib.BrDeviceBam(data.data_ptr(), data.numel(), off.data_ptr(), off.numel())
    t, n = C.c_void_p(), C.c_uint64()
    L = lib.lib()
    L.br_sam_format_device.argtypes = [C.c_void_p, C.POINTER(lib.BrDeviceBam), C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
    rc = L.br_sam_format_device(ctx.h, C.byref(db), None, C.byref(t), C.byref(n))
    torch.cuda.synchronize()
    return rc, n.value


def every_tag():
    t = b"XAAq" + b"Xcc\x80" + b"Ycc\x7f" + b"XCC\x00" + b"YCC\xff" + b"Xss" + struct.pack("<h", -32768) + b"Yss" + struct.pack("<h", 32767)
    t += b"XSS" + struct.pack("<H", 65535) + b"Xii" + struct.pack("<i", -2 ** 31) + b"Yii" + struct.pack("<i", 2 ** 31 - 1)
    t += b"XII" + struct.pack("<I", 2 ** 32 - 1) + b"YII" + struct.pack("<I", 0) + b"Xff" + struct.pack("<f", 0.1)
    t += b"XZZhello world\0" + b"YZZ\0" + b"XHH1AE301\0"
    for sub, fmt_, vals in ((b"c", "b", [-128, 0, 127]), (b"C", "B", [0, 255]), (b"s", "h", [-32768, 32767]), (b"S", "H", [0, 65535]),
                            (b"i", "i", [-2 ** 31, 2 ** 31 - 1, 7]), (b"I", "I", [0, 2 ** 32 - 1]), (b"f", "f", [1.5, -2.25e-7, 3e12])):
        t += b"B" + sub + b"B" + sub + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), fmt_), *vals)
        t += b"E" + sub + b"B" + sub + struct.pack("<I", 0)   # an empty array: B:<sub> with no comma
    return t


def hand_records():
    every_op = [((k * 37 + 1) << 4) | k for k in range(10)] + [((1 << 28) - 1) << 4]
    rng = np.random.RandomState(3)
    recs = [
        bamio.bam_record(b"plain", 0, 99, [(50 << 4) | 0], 50, aux=b"NHC\x01"),
        bamio.bam_record(b"tags", 1, 0, [(20 << 4) | 0, (5 << 4) | 3, (30 << 4) | 0], 50, aux=every_tag(), mate=(1, 400, -451), flag=99),
        bamio.bam_record(b"unplaced", -1, -1, [], 0, flag=4, mapq=0),                                   # RNAME *, POS 0, CIGAR *, SEQ *, QUAL *
        bamio.bam_record(b"past_names", 7, 5, [(3 << 4)], 3, mate=(2, 17, 0)),                         # refID >= n prints *; RNEXT another name
        bamio.bam_record(b"mate_past", 2, 5, [(3 << 4)], 3, mate=(9, 17, 12)),                         # mtid >= n prints *
        bamio.bam_record(b"no_qual", 0, 5, [(5 << 4)], 5, qual=b"\xff" * 5),                           # QUAL 0xff prints *
        bamio.bam_record(b"odd", 0, 5, [(7 << 4)], 7, seq=bytes(rng.randint(0, 256, 4).astype(np.uint8))),   # odd l_seq, every nt16 code
        bamio.bam_record(b"all_codes", 0, 5, [(32 << 4)], 32, seq=bytes(range(0, 256, 17)), qual=bytes(range(0, 96, 3))),
        bamio.bam_record(b"every_op", 0, 5, every_op, 0),                                              # every op code, the longest length
        bamio.bam_record(b"spilled", 0, 1499, [(20 << 4), (10 << 4) | 2, (30 << 4)], 50, aux=b"NMC\x03", spill=True),   # CG restored
        bamio.bam_record(b"kept_cg", 0, 1499, [50 << 4], 50, aux=b"CGBI" + struct.pack("<IIII", 3, 20 << 4, 10 << 4 | 2, 30 << 4)),
        bamio.bam_record(b"x" * 254, 0, 2 ** 31 - 2, [(1 << 4)], 1, mapq=255, mate=(0, -1, -2 ** 31)),
    ]
    return recs


def test_hand_records_match_host_formatter(ctx):
    stream = bamio.frame(hand_records())
    want = records_to_sam_cg(stream, NAMES)
    got = fmt(ctx, stream)
    assert got == want
    lines = got.split(b"\n")
    assert lines[2].split(b"\t")[2:6] == [b"*", b"0", b"0", b"*"] and lines[2].split(b"\t")[9:11] == [b"*", b"*"]
    assert b"\tEc:B:c\t" in got and b"\tBC:B:C,0,255\t" in got and b"\tXi:i:-2147483648\t" in got and b"\tXI:i:4294967295\t" in got
    assert lines[9].split(b"\t")[5] == b"20M10D30M" and b"CG:" not in lines[9]
    assert lines[10].endswith(b"\tCG:B:I,320,162,480")


def test_long_values_and_records(ctx):
    rng = np.random.RandomState(11)
    z = bytes(rng.randint(33, 127, 70000).astype(np.uint8))
    big = struct.pack("<%di" % 300000, *rng.randint(-2 ** 31, 2 ** 31 - 1, 300000).tolist())
    recs = [bamio.bam_record(b"short%d" % k, 0, 10 * k, [(40 << 4)], 40, aux=b"NHC\x02") for k in range(40)]
    recs.insert(5, bamio.bam_record(b"long_z", 0, 7, [(3000 << 4)], 3000, aux=b"ZZZ" + z + b"\0" + b"HHH" + z[:5000].hex().encode() + b"\0"))
    recs.insert(20, bamio.bam_record(b"one_mb", 1, 7, [(90 << 4)] * 300, 27000, aux=b"BBBi" + struct.pack("<I", 300000) + big))
    assert len(recs[20]) > 1 << 20
    stream = bamio.frame(recs)
    assert fmt(ctx, stream) == records_to_sam_cg(stream, NAMES)


def test_empty_stream(ctx):
    assert fmt(ctx, np.zeros(0, np.uint8)) == b""


def test_bad_records_fail_without_text(ctx):
    good = bamio.bam_record(b"ok", 0, 5, [(3 << 4)], 3)
    for aux in (b"XXq\x01", b"XBBf" + struct.pack("<I", 5) + b"\0" * 8, b"XZZunterminated", b"XBBq" + struct.pack("<I", 0), b"Xi"):
        rc, n = raw_rc(ctx, bamio.frame([good, bamio.bam_record(b"bad", 0, 5, [(3 << 4)], 3, aux=aux), good]))
        assert rc == -1 and n == 0, aux
    assert raw_rc(ctx, bamio.frame([good]))[0] == 0


def float_records(bits, per=100000):
    recs = []
    for a in range(0, len(bits), per):
        chunk = np.ascontiguousarray(bits[a:a + per], dtype="<u4")
        recs.append(bamio.bam_record(b"f%d" % a, 0, 5, [(2 << 4)], 2, aux=b"FFBf" + struct.pack("<I", len(chunk)) + chunk.tobytes()))
    return recs


def test_floats_match_glibc(ctx):
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001,
                         0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000], dtype=np.uint32)
    ties = np.array([123456.5, 123457.5, 1234565, 999999.5, 1e-45, 0.0001, 0.00001, 99999.95, 999999, 1e6, 1e-5, 9.999995e-5,
                     0.5, 2.5, 1e38, 3.4028235e38, 1.17549435e-38, 100000, 123456, 0.1, 1.0 / 3], dtype=np.float32).view(np.uint32)
    rng = np.random.RandomState(2026)
    rnd = rng.randint(0, 2 ** 32, size=10_000_000, dtype=np.uint64).astype(np.uint32)
    # short records with f tags and small arrays (16 lanes each), long ones with 100 000 values (a wave each)
    short = [bamio.bam_record(b"s%d" % k, 0, 5, [(2 << 4)], 2, aux=b"XFf" + struct.pack("<I", int(v)) + b"YFBf" + struct.pack("<I", 3) +
                              np.array([v, ~v & 0xffffffff, v ^ 1], dtype="<u4").tobytes()) for k, v in enumerate(np.concatenate([specials, ties]))]
    stream = bamio.frame(short + float_records(np.concatenate([specials, ties, rnd])))
    got = fmt(ctx, stream)
    want = synth.records_to_sam(stream, NAMES)
    assert got.count(b",") >= 10_000_000
    if got != want:
        a, b = got.split(b"\n"), want.split(b"\n")
        for x, y in zip(a, b):
            if x != y:
                xs, ys = x.split(b","), y.split(b",")
                bad = [(i, p, q) for i, (p, q) in enumerate(zip(xs, ys)) if p != q][:5]
                raise AssertionError("first differences (index, device, glibc): %r" % bad)
        raise AssertionError("line counts differ")
    line = got.split(b"\n")[len(specials) + 0]
    assert line.split(b"\t")[11] == b"XF:f:123456"
    text = {v: got.split(b"\n")[len(specials) + k].split(b"\t")[11][5:] for k, v in enumerate([123456.5, 123457.5, 1234565, 999999.5, 1e-45])}
    assert text == {123456.5: b"123456", 123457.5: b"123458", 1234565: b"1.23456e+06", 999999.5: b"1e+06", 1e-45: b"1.4013e-45"}
    assert [got.split(b"\n")[k].split(b"\t")[11][5:] for k in (0, 1, 2, 3, 4, 5)] == [b"0", b"-0", b"inf", b"-inf", b"nan", b"-nan"]


def test_bundle_entry_points_with_sam_text():
    """the bundle path (records -> projection -> re-encoding -> text), host and resident forms, against the text of the BAM path"""
    import torch
    ann = synth.Annotation("G", n_genes=400, n_refs=3)
    annd = ann.as_dict()
    b = ann.reads(3000, "pe", with_records=1, xs_tag=True)
    stream, roff, rlen = synth.Annotation.frame_records(b)
    idx = lib.Index(annd, device=0)
    ctx = lib.Context(idx)
    names = [idx.transcript_name(t) for t in range(idx.num_transcripts())]
    ctx.set_sam_refs(names)
    rm = np.arange(ann.n_refs, dtype=np.int32)
    cfg = lib.make_config()
    bam, cnt = ctx.project_bam_bundle(cfg, stream, roff, rlen, rm)
    sam, cnt2 = ctx.project_bam_bundle(cfg, stream, roff, rlen, rm, sam_text=True)
    assert cnt == cnt2 and cnt["n_rows"] > 3000
    assert bytes(sam) == records_to_sam_py(bam, names)
    recs = lib.BrDeviceRecords()
    d_blob = torch.from_numpy(stream.copy()).to("cuda:0")
    d_off = torch.from_numpy(np.asarray(roff, dtype=np.int64)).to("cuda:0")
    d_len = torch.from_numpy(np.asarray(rlen, dtype=np.int32)).to("cuda:0")
    recs.blob, recs.rec_off, recs.n_aln, recs.rec_len = d_blob.data_ptr(), d_off.data_ptr(), len(rlen), d_len.data_ptr()
    sam2, cnt3 = ctx.project_bam_resident(cfg, recs, rm, sam_text=True)
    assert bytes(sam2) == bytes(sam) and cnt3 == cnt
    ctx.close()
    idx.close()


# ---- the command line -------------------------------------------------------------------------------------------------------
def cli_pair(tmp_path, in_path, gtf, flags, fasta=None):
    """the same run twice, BAM and -O sam: (sam bytes, expected bytes from the BAM, BAM records, BAM reference names)"""
    out_bam, out_sam = str(tmp_path / "out.bam"), str(tmp_path / "out.sam")
    base = [BIN, in_path, "-G", gtf, "-p", "4", "--bundle-size", "1500"] + (["-S", fasta] if fasta else []) + flags
    cmd_bam, cmd_sam = base + ["-o", out_bam], base + ["-o", out_sam, "--output-fmt", "SAM"]
    for cmd in (cmd_bam, cmd_sam):
        r = subprocess.run(cmd, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode() + r.stdout.decode()
    text, refs, recs = bamio.read_bam(out_bam)
    names = [n for n, _ in refs]
    header = text.replace(" ".join(cmd_bam), " ".join(cmd_sam)).encode()   # (the @PG line's CL: differs)
    with open(out_sam, "rb") as f:
        sam = f.read()
    return sam, header + records_to_sam_cg(recs, names), recs, names


def short_read_inputs(tmp_path, shuffle=False):
    ann = synth.Annotation("G", n_genes=800, n_refs=4)
    annd = ann.as_dict()
    b = ann.reads(5000, "pe", with_records=1, xs_tag=True)
    stream = framed_stream(b, unmapped_every=101)
    if shuffle:
        recs = bamio.split_stream(stream)
        perm = np.random.RandomState(9).permutation(len(recs))
        stream = bamio.frame([recs[i] for i in perm])
    gtf = str(tmp_path / "guides.gtf")
    bamio.write_gtf(gtf, annd)
    bam_refs = [(n, 1000000) for n in annd["refnames"]]
    hdr = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bam_refs) + "@PG\tID:aligner\tPN:aligner\n"
    in_bam = str(tmp_path / "in.bam")
    bamio.write_bam(in_bam, hdr, bam_refs, stream.tobytes(), block=40000)
    return in_bam, gtf, stream, hdr, annd


@pytest.mark.parametrize("flags", [["--device-reader"], ["--host-reader"], ["--devices", "0,0"]])
def test_cli_sam_equals_bam_text(tmp_path, flags):
    in_bam, gtf, _, _, _ = short_read_inputs(tmp_path)
    sam, want, recs, _ = cli_pair(tmp_path, in_bam, gtf, flags)
    assert sam.count(b"\n") > 5000 and sam == want
    assert not [p for p in os.listdir(tmp_path) if "tmp-bramble" in p]


def test_cli_sam_collate_and_round_trip(tmp_path):
    in_bam, gtf, _, _, _ = short_read_inputs(tmp_path, shuffle=True)
    sam, want, recs, names = cli_pair(tmp_path, in_bam, gtf, ["--collate"])
    assert sam == want
    # encoding the lines back gives the BAM run's records, up to bin and the integer widths of the tags
    body = b"".join(l + b"\n" for l in sam.split(b"\n") if l and not l.startswith(b"@"))
    _, _, every = encode_sam(body, names)
    a, b = bamio.split_stream(recs), bamio.split_stream(every)
    assert len(a) == len(b) > 5000
    for r1, r2 in zip(a, b):
        f1, f2 = bamio.record_fields(r1), bamio.record_fields(r2)
        for k in ("ref_id", "pos", "name", "mapq", "flag", "l_seq", "mtid", "mpos", "tlen", "cigar", "seq", "qual"):
            assert f1[k] == f2[k], k
    assert records_to_sam_py(every, names) == body


def test_cli_sam_from_sam_input_and_to_stdout(tmp_path):
    in_bam, gtf, stream, hdr, annd = short_read_inputs(tmp_path)
    in_sam = str(tmp_path / "in.sam")
    with open(in_sam, "wb") as f:
        f.write(hdr.encode() + synth.records_to_sam(stream, annd["refnames"]))
    sam, want, _, _ = cli_pair(tmp_path, in_sam, gtf, [])
    assert sam == want
    _, want2, _, _ = cli_pair(tmp_path, in_bam, gtf, [])
    r = subprocess.run([BIN, in_bam, "-G", gtf, "-p", "4", "--bundle-size", "1500", "-o", "-", "-O", "sam"], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    co = lambda t: t.index(b"@CO\tGenerated")   # (from the @CO line on: the @PG line's CL: differs)
    assert r.stdout[co(r.stdout):] == want2[co(want2):] and r.stdout[:co(r.stdout)].count(b"\n") == want2[:co(want2)].count(b"\n")


def test_cli_sam_long_reads_with_tags(tmp_path):
    ann = synth.Annotation("G", n_genes=200, n_refs=2, with_genome=True)
    annd = ann.as_dict()
    b = ann.reads(1500, "ont", with_seq=1, with_records=1)
    rng = np.random.RandomState(4)
    recs = []
    for r in bamio.split_stream(framed_stream(b)):
        fl = rng.randint(0, 2 ** 32, 5, dtype=np.uint64).astype("<u4")
        recs.append(r + b"XFf" + fl[:1].tobytes() + b"XBBf" + struct.pack("<I", 4) + fl[1:].tobytes() + b"XHH0A1B2C\0" + b"XAAz" +
                    b"XZZ" + bytes(rng.randint(65, 91, 2500).astype(np.uint8)) + b"\0")
    fasta = str(tmp_path / "genome.fa")
    with open(fasta, "w") as f:
        for rid, name in enumerate(annd["refnames"]):
            seq = annd["ref_seqs"][rid]
            seq = bytes(seq).decode() if isinstance(seq, (bytes, bytearray)) else seq
            f.write(">%s\n" % name + "".join(seq[a:a + 70] + "\n" for a in range(0, len(seq), 70)))
    gtf = str(tmp_path / "guides.gtf")
    bamio.write_gtf(gtf, annd)
    bam_refs = [(n, len(annd["ref_seqs"][i])) for i, n in enumerate(annd["refnames"])]
    in_bam = str(tmp_path / "in.bam")
    bamio.write_bam(in_bam, "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in bam_refs), bam_refs, bamio.frame(recs).tobytes(), block=40000)
    sam, _, out_recs, names = cli_pair(tmp_path, in_bam, gtf, ["--lr"], fasta=fasta)
    assert sam.count(b"\n") > 1000 and b"\tXB:B:f," in sam and b"\tXA:A:z" in sam and b"\tXH:H:0A1B2C" in sam
    # glibc's %g for the f values: the C++ host formatter
    body = sam[sam.index(b"\n", sam.index(b"@CO\tGenerated")) + 1:]
    assert body == synth.records_to_sam(out_recs, names)


def test_cli_sam_ultra_long_cigar(tmp_path):
    cig, qlen, _ = long_cigar(17501)   # 70004 ops: spilled into CG:B,I in the BAM, printed as the CIGAR in the text
    recs = [bamio.bam_record(b"r%02d" % i, 0, 1200 + 37 * i, [(90 << 4)], 90, aux=b"NMC\x01") for i in range(30)]
    recs.insert(10, bamio.bam_record(b"ultra", 0, 1999, cig, qlen, aux=b"NMi" + struct.pack("<i", 5)))
    gtf = str(tmp_path / "guides.gtf")
    bamio.write_gtf(gtf, ANN)
    in_bam = str(tmp_path / "in.bam")
    bamio.write_bam(in_bam, "@SQ\tSN:chr1\tLN:400000\n", [("chr1", 400000)], bamio.frame(recs).tobytes())
    sam, want, out_recs, _ = cli_pair(tmp_path, in_bam, gtf, ["--lr"])
    assert sam == want
    long_lines = [l for l in sam.split(b"\n") if l.startswith(b"ultra")]
    assert len(long_lines) == 2 and all(b"CG:" not in l and len(l.split(b"\t")[5]) > 4 * 17501 for l in long_lines)


def test_cli_missing_guides_leave_no_sam(tmp_path):
    in_bam, _, _, _, _ = short_read_inputs(tmp_path)
    out = str(tmp_path / "x.sam")
    r = subprocess.run([BIN, in_bam, "-G", str(tmp_path / "missing.gtf"), "-o", out, "-O", "sam"], capture_output=True, timeout=600)
    assert r.returncode != 0 and not os.path.exists(out) and not os.path.exists(out + ".tmp-bramble")

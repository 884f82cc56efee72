"""SAM text input on the GPU: br_sam_reader's records byte for byte against the tests' own encoder (tests/test_sam_cpu.py,
written from htslib's sam_parse1 + bam_write1 rules), chunking at read-name groups, and the command line on SAM files and
SAM on standard input against the same records as BAM."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

from bramble_amd import lib, synth
from oracle import oracle_binding as ob
from tests import bamio
from tests.test_gpu_bam_bundle import framed_stream
from tests.test_sam_cpu import encode_sam

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bramble_amd", "bin", "bramble")

REFS = [("chr1", 5000000), ("chr2", 300000)]
HEADER = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@CO\tcomment\twith\ttabs\n"


def hand_lines():
    """One line (or a few) per rule of the byte contract."""
    L = []
    q = lambda n: "I" * n
    base = "%s\t%d\tchr1\t%d\t60\t%s\t*\t0\t0\t%s\t%s"
    # integer tag boundaries: the smallest type that holds the value
    ints = [-129, -128, -32769, -32768, 255, 256, 65535, 65536, 2 ** 32 - 1, -2 ** 31, 0, 127, 128]
    L.append(base % ("int", 0, 100, "10M", "ACGTACGTAC", q(10)) + "".join("\tX%d:i:%d" % (k % 10, v) for k, v in enumerate(ints)))
    # floats: on the device's fast path and off it (25-digit mantissa, subnormal, double rounding differs from single)
    fl = ["0.1", "-3.25", "12e3", "5E-2", "1", "-0", "0.000123", "1.234567890123456789012345", "1e-40", "1.0000000596046448",
          "3.4028235e38", "1e22", "123456789012345678"]
    L.append(base % ("flt", 0, 200, "10M", "ACGTACGTAC", q(10)) + "".join("\tf%d:f:%s" % (k % 10, v) for k, v in enumerate(fl)) +
             "\tBf:B:f," + ",".join(fl) + "\tBc:B:c,-128,127\tBC:B:C,0,255\tBs:B:s,-32768,32767\tBS:B:S,65535\tBi:B:i,-2147483648\tBI:B:I,4294967295\tBe:B:i")
    L.append(base % ("hz", 0, 300, "4M", "ACGT", q(4)) + "\tHH:H:1AE301\tZZ:Z:text with spaces\tAA:A:x\tZe:Z:" +
             "\tMM:Z:" + "C+m," * 2000 + "\tXX:i:5\tHL:H:" + "0A" * 700)   # long Z / H values: copied by the whole wave
    # SEQ / QUAL
    L.append(base % ("seqstar", 0, 400, "5M", "*", "*"))
    L.append(base % ("qualstar", 0, 400, "5M", "AcG=n", "*"))
    L.append(base % ("lower", 0, 400, "3S6M1I", "acgtnRYKMS", "!#%&()*+,-"))
    L.append(base % ("odd", 16, 400, "2M1D3M2N2M", "ACGTTGG", "ABCDEFG"))
    # RNAME / RNEXT
    L.append("mate1\t1\tchr1\t500\t30\t5M\t=\t700\t205\tACGTA\tIIIII")
    L.append("mate2\t1\tchr1\t500\t30\t5M\t*\t0\t0\tACGTA\tIIIII")
    L.append("mate3\t1\tchr1\t500\t30\t5M\tchr2\t9\t0\tACGTA\tIIIII")
    L.append("mate4\t1\tchr2\t500\t30\t5M\tchrNope\t9\t0\tACGTA\tIIIII")
    L.append("unk\t0\tchrNope\t500\t30\t5M\t*\t0\t0\tACGTA\tIIIII")          # unknown RNAME: unmapped
    L.append("f4\t4\tchr1\t500\t0\t5M\t*\t0\t0\tACGTA\tIIIII")               # flag 4
    L.append("nocig\t0\tchr1\t500\t0\t*\t*\t0\t0\tACGTA\tIIIII")             # mapped without CIGAR: unmapped
    L.append("hard\t0\tchr1\t500\t0\t5H\t*\t0\t0\t*\t*")                      # no query-consuming op: unmapped
    L.append("pos0\t0\tchr2\t1\t0\t3M\t*\t0\t0\tAAA\tIII")
    L.append("bigpos\t0\tchr1\t4999990\t0\t3M100000N3M\t*\t0\t-12\tAAAAAA\tIIIIII")
    # 70 000 CIGAR ops: the CG:B,I form
    ops = "1M1I" * 35000
    ql = 70000
    L.append("longcig\t0\tchr1\t1000\t60\t%s\t*\t0\t0\t%s\t%s\tNM:i:3" % (ops, "A" * ql, "J" * ql))
    # a 200 kB line
    n = 100000
    L.append("ultralong\t0\tchr2\t10\t60\t%dS%dM\t*\t0\t0\t%s\t%s\tde:f:0.0123\tMM:Z:C+m,1,2" % (100, n - 100, ("ACGTN" * (n // 5)), ("+5?" * (n // 3 + 1))[:n]))
    return L


def reader_records(text, last=True, header=HEADER, device=0):
    r = lib.SamReader(header, device=device)
    try:
        return r.next(text, last)
    finally:
        r.close()


def test_sam_records_byte_for_byte_hand_lines():
    lines = hand_lines()
    text = ("\n".join(lines[:5]) + "\r\n" + "\r\n".join(lines[5:9]) + "\n" + "\n".join(lines[9:])).encode()   # CRLF, no final '\n'
    exp, n_un, _ = encode_sam(text, [r[0] for r in REFS])
    got = reader_records(text, last=True)
    assert got["consumed"] == len(text)
    assert got["n_unmapped"] == n_un == 4
    assert got["n"] == len(lines) - 4
    assert got["stream"].size == exp.size and np.array_equal(got["stream"], exp)


@pytest.mark.parametrize("mode", ["pe", "ont"])
def test_sam_records_byte_for_byte_synthetic(mode):
    ann = synth.Annotation("G", n_genes=400, n_refs=2, with_genome=(mode == "ont"))
    names = ann.as_dict()["refnames"]
    b = ann.reads(3000 if mode == "pe" else 400, mode, with_records=1, xs_tag=True)
    text = synth.records_to_sam(framed_stream(b, unmapped_every=17), names)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, 10 ** 7) for n in names)
    exp, n_un, _ = encode_sam(text, names)
    got = reader_records(text, last=True, header=header)
    assert got["n_unmapped"] == n_un and n_un > 0
    assert np.array_equal(got["stream"], exp)


def _names(stream):
    s, p, out = bytes(stream), 0, []
    while p < len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        out.append(s[p + 36:p + 36 + s[p + 12] - 1])
        p += 4 + bs
    return out


def test_sam_chunking_at_read_name_groups():
    ann = synth.Annotation("G", n_genes=300, n_refs=2)
    names = ann.as_dict()["refnames"]
    b = ann.reads(1500, "pe", with_records=1)
    text = synth.records_to_sam(framed_stream(b, unmapped_every=9), names)
    header = "".join("@SQ\tSN:%s\tLN:%d\n" % (n, 10 ** 7) for n in names)
    exp, n_un, _ = encode_sam(text, names)
    whole = None
    for piece in (1000, 70000, len(text)):
        r = lib.SamReader(header)
        try:
            parts, un, pos, end, zero = [], 0, 0, min(piece, len(text)), 0
            while True:
                last = end >= len(text)
                got = r.next(text[pos:end], last)
                un += got["n_unmapped"]
                if got["n"]:
                    parts.append(got["stream"])
                if got["consumed"] == 0 and not last:
                    zero += 1
                    end = min(len(text), end + piece)
                    continue
                pos += got["consumed"]
                if last:
                    assert pos == len(text)
                    break
                end = min(len(text), pos + piece)
            # every bundle ends at a read-name change
            for a, b2 in zip(parts, parts[1:]):
                assert _names(a)[-1] != _names(b2)[0]
            cat = np.concatenate(parts)
            assert np.array_equal(cat, exp) and un == n_un, piece
            if piece == 1000:
                assert zero > 0 and len(parts) > 100
            whole = cat
        finally:
            r.close()
    # one group longer than the piece: nothing is consumed
    first = text.split(b"\n")[1] + b"\n"   # (line 0 is an unmapped copy)
    r = lib.SamReader(header)
    try:
        assert r.next(first, False)["consumed"] == 0
    finally:
        r.close()
    assert whole is not None


# ---- command line ---------------------------------------------------------------------------------------------------------
def _write_inputs(tmp_path, annd, stream, header, fasta=False):
    names = annd["refnames"]
    text = synth.records_to_sam(stream, names)
    _, _, every = encode_sam(text, names)   # the equivalent BAM: the same lines as htslib would store them
    refs = [(n, len(annd["ref_seqs"][i]) if fasta else 10 ** 7) for i, n in enumerate(names)]
    hdr = header + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
    sam, bam, gtf = str(tmp_path / "in.sam"), str(tmp_path / "in.bam"), str(tmp_path / "g.gtf")
    open(sam, "wb").write(hdr.encode() + text)
    bamio.write_bam(bam, hdr, refs, every.tobytes(), block=40000)
    bamio.write_gtf(gtf, annd)
    fa = None
    if fasta:
        fa = str(tmp_path / "genome.fa")
        with open(fa, "w") as f:
            for rid, name in enumerate(names):
                seq = annd["ref_seqs"][rid]
                seq = bytes(seq).decode() if isinstance(seq, (bytes, bytearray)) else seq
                f.write(">%s\n" % name)
                for a in range(0, len(seq), 70):
                    f.write(seq[a:a + 70] + "\n")
    return sam, bam, gtf, fa, every


def _run(args, out, stdin=None, timeout=600, fifo=None):
    cmd = [BIN] + args + ["-o", out]
    if fifo:   # the input as a path that is a pipe: bash's <(cat file)
        cmd = ["bash", "-c", '"$0" <(cat "$1") "${@:2}"', BIN, fifo] + args + ["-o", out]
    r = subprocess.run(cmd, input=stdin, capture_output=True, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode() + r.stdout.decode()
    return r.stdout.decode()


def _report(stdout):
    return [l for l in stdout.split("\n") if l.startswith("# ")]


@pytest.mark.parametrize("mode", ["pe", "lr"])
def test_cli_sam_equals_bam(tmp_path, mode):
    ann = synth.Annotation("G", n_genes=600, n_refs=3, with_genome=(mode == "lr"))
    annd = ann.as_dict()
    b = ann.reads(4000 if mode == "pe" else 1500, "pe" if mode == "pe" else "ont", with_records=1, xs_tag=True,
                  **({"with_seq": 1} if mode == "lr" else {}))
    stream = framed_stream(b, unmapped_every=31)
    sam, bam, gtf, fa, every = _write_inputs(tmp_path, annd, stream, "@HD\tVN:1.6\n@PG\tID:aligner\tPN:aligner\n", fasta=(mode == "lr"))
    extra = ["-G", gtf, "--compression-level", "1"] + (["--lr", "-S", fa] if mode == "lr" else [])
    o_bam, o_sam, o_pipe, o_two, o_small, o_fsam, o_fbam = (str(tmp_path / x) for x in ("o_bam.bam", "o_sam.bam", "o_pipe.bam", "o_two.bam",
                                                                                      "o_small.bam", "o_fifo_sam.bam", "o_fifo_bam.bam"))
    rep_bam = _report(_run([bam] + extra, o_bam))
    rep_sam = _report(_run([sam] + extra, o_sam))
    rep_pipe = _report(_run(["-"] + extra, o_pipe, stdin=open(sam, "rb").read()))
    rep_two = _report(_run([sam, "--devices", "0,0"] + extra, o_two))
    rep_small = _report(_run([sam, "--bundle-size", "2500"] + extra, o_small))
    rep_fsam = _report(_run(extra, o_fsam, fifo=sam))   # a pipe given by its path: nothing of its start may be lost
    rep_fbam = _report(_run(extra, o_fbam, fifo=bam))
    t0, r0, s0 = bamio.read_bam(o_bam)
    assert len(s0) > 100000
    # the records against the oracle (transcripts in guide order, the input's references in annotation order)
    order = bamio.guide_order(annd)
    sorted_ann = dict(annd)
    sorted_ann["transcripts"] = [annd["transcripts"][t] for t in order]
    roff, rlen, _, _ = lib.bam_split(every)
    flags = ob.make_flags(**({"lr": 1, "use_fasta": 1} if mode == "lr" else {}))
    orc, _, _, _ = ob.run_bam(ob.OracleIndex(sorted_ann), flags, every, roff, rlen, np.arange(len(annd["refnames"]), dtype=np.int32))
    assert np.array_equal(s0, orc["bam_stream"])
    for o in (o_sam, o_pipe, o_two, o_small, o_fsam, o_fbam):
        t, r, s = bamio.read_bam(o)
        # the header differs only in the @PG command line
        strip = lambda x: [l for l in x.split("\n") if not l.startswith("@PG\tID:bramble")]
        assert strip(t) == strip(t0) and r == r0 and np.array_equal(s, s0), o
    for rep in (rep_sam, rep_pipe, rep_two, rep_small, rep_fsam, rep_fbam):
        assert rep == rep_bam and len(rep) == 5


def _err_run(tmp_path, body, name="bad.sam", raw=None):
    gtf = str(tmp_path / "g.gtf")
    open(gtf, "w").write('chr1\tx\texon\t10\t500\t.\t+\t.\tgene_id "g"; transcript_id "t1";\n')
    path = str(tmp_path / name)
    open(path, "wb").write(raw if raw is not None else (HEADER + body).encode())
    out = str(tmp_path / "out.bam")
    r = subprocess.run([BIN, path, "-G", gtf, "-o", out], capture_output=True, timeout=300)
    assert r.returncode != 0
    assert not os.path.exists(out) and not os.path.exists(out + ".tmp-bramble")
    return r.stderr.decode()


GOOD = "r%d\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\n"


@pytest.mark.parametrize("bad,why", [
    ("r9\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\n", "fewer than 11 fields"),
    ("r9\t0\tchr1\t100\t60\t4Q\t*\t0\t0\tACGT\tIIII\n", "CIGAR"),
    ("r9\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIII\n", "QUAL length"),
    ("r9\t0\tchr1\t100\t60\t5M\t*\t0\t0\tACGT\tIIII\n", "SEQ length"),
    ("r9\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXI:i:4294967296\n", "out of range"),
    ("r9\t4\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXf:f:1.5x\n", "float"),   # on an unmapped line too
    ("r9\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXf:f:2e\n", "float"),
])
def test_cli_sam_errors_name_the_line(tmp_path, bad, why):
    body = "".join(GOOD % k for k in range(5)) + bad + "".join(GOOD % k for k in range(10, 14))
    err = _err_run(tmp_path, body)
    line = HEADER.count("\n") + 6
    assert ("bad.sam:%d: " % line) in err and why in err, err


def test_cli_rejects_bgzipped_sam_and_gzip(tmp_path):
    text = (HEADER + GOOD % 1).encode()
    err = _err_run(tmp_path, None, name="bgz.sam.gz", raw=bamio.bgzf_compress(text))
    assert "BGZF-compressed SAM" in err, err
    err = _err_run(tmp_path, None, name="plain.sam.gz", raw=gzip.compress(text))
    assert "gzip" in err, err


def test_sam_malformed_floats_are_errors_of_their_own_line():
    """A float strtod does not take whole is an error of the line that holds it, mapped or not, and the first such line is the
    one reported even when a later line fails in another way."""
    good = GOOD % 1
    cases = [("r2\t4\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXf:f:nanx\n", 2),
             ("r2\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXf:B:f,1,0x\n", 2),
             ("r2\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII\tXf:f:1e+\n" + "r3\t0\tchr1\n", 2)]
    for body, line in cases:
        with pytest.raises(lib.SamError) as e:
            reader_records((good + body).encode(), last=True)
        assert e.value.line == line, (body, e.value)
    # what strtod takes whole is accepted: white space in front, inf / nan, hex
    ok = good.rstrip("\n") + "\tXa:f: 1.5\tXb:f:-inf\tXc:f:NaN\tXd:f:0x1.8p1\tXe:B:f,infinity,0X10\n"
    exp, n_un, _ = encode_sam(ok.encode(), [r[0] for r in REFS])
    got = reader_records(ok.encode(), last=True)
    assert np.array_equal(got["stream"], exp) and n_un == 0

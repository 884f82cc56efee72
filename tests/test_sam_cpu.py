"""SAM input without a GPU: the C ABI's new symbols, br_sam_header_scan, the C++ BAM -> SAM writer against a Python one.
The module also holds the tests' own SAM -> BAM encoder (encode_sam), written from the rules htslib's sam_parse1 +
bam_write1 follow (restated in bramble_amd/csrc/sam_kernels.hip) and independent of the HIP code: the GPU tests
(tests/test_gpu_sam.py) take their expected bytes from it."""
import ctypes as C
import re
import struct

import numpy as np

from bramble_amd import lib, synth
from tests.test_gpu_bam_bundle import framed_stream

# htslib's seq_nt16_table: '=' 0, ACMGRSVTWYHKDBN 1..15 in either case, U 8, the digits 0-3 -> 1 2 4 8, anything else 15
NT16 = [15] * 256
for _i, _c in enumerate("=ACMGRSVTWYHKDBN"):
    NT16[ord(_c)] = _i
    NT16[ord(_c.lower())] = _i
NT16[ord("U")] = NT16[ord("u")] = 8
for _i, _c in enumerate("0123"):
    NT16[ord(_c)] = (1, 2, 4, 8)[_i]
NT16[ord("=")] = 0

CIGAR_OPS = "MIDNSHP=X"


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def _int_tag(v):
    if v < -2 ** 31 or v > 2 ** 32 - 1:
        raise ValueError("i tag out of range")
    if v < 0:
        return (b"c", struct.pack("<b", v)) if v >= -128 else (b"s", struct.pack("<h", v)) if v >= -32768 else (b"i", struct.pack("<i", v))
    return (b"C", struct.pack("<B", v)) if v <= 255 else (b"S", struct.pack("<H", v)) if v <= 65535 else (b"I", struct.pack("<I", v))


def _f32(text):
    t = text.decode() if isinstance(text, bytes) else text
    d = float.fromhex(t) if "x" in t.lower() else float(t)
    return np.float32(d).tobytes()   # (float)strtod(text): double first, then float


def encode_tag(t):
    tag, ty, val = t[:2], t[3:4], t[5:]
    assert t[2:3] == b":" and t[4:5] == b":"
    if ty == b"A":
        assert len(val) == 1
        return tag + b"A" + val
    if ty == b"i":
        c, b = _int_tag(int(val))
        return tag + c + b
    if ty == b"f":
        return tag + b"f" + _f32(val)
    if ty in (b"Z", b"H"):
        return tag + ty + val + b"\0"
    if ty == b"B":
        sub = val[:1]
        vals = val[2:].split(b",") if len(val) > 1 else []
        fmt = {b"c": "b", b"C": "B", b"s": "h", b"S": "H", b"i": "i", b"I": "I"}
        body = b"".join(_f32(v) if sub == b"f" else struct.pack("<" + fmt[sub], int(v)) for v in vals)
        return tag + b"B" + sub + struct.pack("<I", len(vals)) + body
    raise ValueError("tag type")


def encode_line(line, refs):
    """One SAM line (bytes, no newline) -> (BAM record with its block_size, mapped?)."""
    f = line.split(b"\t")
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    ref = -1 if rname == b"*" else refs.get(rname, -1)
    nref = ref if rnext == b"=" else -1 if rnext == b"*" else refs.get(rnext, -1)
    ops = [] if cigar == b"*" else [(int(n), CIGAR_OPS.index(c.decode())) for n, c in re.findall(rb"(\d+)([MIDNSHP=X])", cigar)]
    qlen = sum(n for n, o in ops if o in (0, 1, 4, 7, 8))
    rlen = sum(n for n, o in ops if o in (0, 2, 3, 7, 8))
    flag = int(flag)
    if ref < 0 or qlen == 0:
        flag |= 4
    l_seq = 0 if seq == b"*" else len(seq)
    seqb = bytes((NT16[seq[2 * k]] << 4) | (NT16[seq[2 * k + 1]] if 2 * k + 1 < l_seq else 0) for k in range((l_seq + 1) // 2))
    qualb = b"\xff" * l_seq if qual == b"*" else bytes(c - 33 for c in qual)
    aux = b"".join(encode_tag(t) for t in f[11:])
    words = [n << 4 | o for n, o in ops]
    if len(words) > 65535:   # bam_write1: <l_seq>S<rlen>N, the real ops in CG:B,I behind the other tags
        aux += b"CGBI" + struct.pack("<I", len(words)) + struct.pack("<%dI" % len(words), *words)
        words = [l_seq << 4 | 4, rlen << 4 | 3]
    pos0 = int(pos) - 1
    # bin is a 16-bit field (bam1_core_t.bin is uint16_t): past 2^29 the record keeps reg2bin's 16 low bits
    rec = struct.pack("<iiBBHHHIiii", ref, pos0, len(qname) + 1, int(mapq), reg2bin(pos0, pos0 + (rlen or 1)) & 0xffff, len(words), flag,
                      l_seq, nref, int(pnext) - 1, int(tlen))
    rec += qname + b"\0" + struct.pack("<%dI" % len(words), *words) + seqb + qualb + aux
    return struct.pack("<I", len(rec)) + rec, not (flag & 4)


def encode_sam(text, ref_names):
    """SAM record lines -> (uint8 stream of the mapped records, number of unmapped lines, uint8 stream of every record)."""
    refs = {n.encode() if isinstance(n, str) else n: i for i, n in reversed(list(enumerate(ref_names)))}
    mapped, every, n_un = [], [], 0
    for line in text.split(b"\n"):
        if not line:
            continue
        line = line[:-1] if line.endswith(b"\r") else line
        rec, ok = encode_line(line, refs)
        every.append(rec)
        if ok:
            mapped.append(rec)
        else:
            n_un += 1
    as_u8 = lambda x: np.frombuffer(b"".join(x), dtype=np.uint8)
    return as_u8(mapped), n_un, as_u8(every)


def records_to_sam_py(stream, ref_names):
    """BAM records -> SAM text, written the way `samtools view` prints them (independent of synth.records_to_sam)."""
    s = bytes(np.asarray(stream, dtype=np.uint8))
    out, p = [], 0
    name = lambda r: ref_names[r] if 0 <= r < len(ref_names) else "*"
    while p + 4 <= len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        r = s[p + 4:p + 4 + bs]
        p += 4 + bs
        rid, pos, lqn, mapq, _bin, ncig, flag, l_seq, nrid, npos, tlen = struct.unpack_from("<iiBBHHHIiii", r, 0)
        q = 32
        qn = r[q:q + lqn - 1].decode()
        q += lqn
        cig = "".join("%d%s" % (w >> 4, "MIDNSHP=XB"[min(w & 15, 9)]) for w in struct.unpack_from("<%dI" % ncig, r, q)) or "*"
        q += 4 * ncig
        seq = "".join("=ACMGRSVTWYHKDBN"[(r[q + (k >> 1)] >> (4 * (1 - (k & 1)))) & 15] for k in range(l_seq)) or "*"
        q += (l_seq + 1) // 2
        qual = "*" if l_seq == 0 or r[q] == 0xff else "".join(chr(c + 33) for c in r[q:q + l_seq])
        q += l_seq
        fields = [qn, str(flag), name(rid), str(pos + 1), str(mapq), cig, "*" if nrid < 0 else "=" if nrid == rid else name(nrid),
                  str(npos + 1), str(tlen), seq, qual]
        isz = {"c": ("b", 1), "C": ("B", 1), "s": ("h", 2), "S": ("H", 2), "i": ("i", 4), "I": ("I", 4)}
        while q + 3 <= len(r):
            tag, t = r[q:q + 2].decode(), chr(r[q + 2])
            q += 3
            if t == "A":
                fields.append("%s:A:%s" % (tag, chr(r[q])))
                q += 1
            elif t in isz:
                fmt, w = isz[t]
                fields.append("%s:i:%d" % (tag, struct.unpack_from("<" + fmt, r, q)[0]))
                q += w
            elif t == "f":
                fields.append("%s:f:%g" % (tag, struct.unpack_from("<f", r, q)[0]))
                q += 4
            elif t in "ZH":
                e = r.index(b"\0", q)
                fields.append("%s:%s:%s" % (tag, t, r[q:e].decode()))
                q = e + 1
            elif t == "B":
                sub, cnt = chr(r[q]), struct.unpack_from("<I", r, q + 1)[0]
                q += 5
                vals = []
                for _ in range(cnt):
                    if sub == "f":
                        vals.append("%g" % struct.unpack_from("<f", r, q)[0])
                        q += 4
                    else:
                        fmt, w = isz[sub]
                        vals.append("%d" % struct.unpack_from("<" + fmt, r, q)[0])
                        q += w
                fields.append("%s:B:%s" % (tag, ",".join([sub] + vals)))
        out.append("\t".join(fields) + "\n")
    return "".join(out).encode()


def test_sam_symbols_exported_and_no_device():
    L = lib.lib()
    for name in ("br_sam_header_scan", "br_sam_reader_new", "br_sam_reader_next", "br_sam_reader_upload", "br_sam_reader_next_staged",
                 "br_sam_reader_release", "br_sam_reader_free",
                 "br_sam_reader_error", "br_sam_reader_stats"):
        assert hasattr(L, name) and name in lib.EXPORTS, name
    L.br_sam_reader_new.argtypes = [C.c_int, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    hdr = b"@SQ\tSN:chr1\tLN:100\n"
    assert L.br_sam_reader_new(99, hdr, len(hdr), C.byref(h)) == -2 and not h.value   # BR_ERR_NO_DEVICE
    try:
        import torch
        have_gpu = torch.cuda.is_available()
    except ImportError:
        have_gpu = False
    if not have_gpu:
        assert L.br_sam_reader_new(0, hdr, len(hdr), C.byref(h)) == -2 and not h.value


def test_sam_header_scan():
    hdr = b"@HD\tVN:1.6\n@SQ\tSN:chr1\tLN:1000\n@CO\tfree\ttext\twith tabs\n"
    rec = b"r1\t0\tchr1\t1\t60\t4M\t*\t0\t0\tACGT\tIIII\n"
    assert lib.sam_header_scan(hdr) == len(hdr)                # header only
    assert lib.sam_header_scan(rec + rec) == 0                 # no header
    assert lib.sam_header_scan(hdr + rec) == len(hdr)          # @CO with tabs, then records
    assert lib.sam_header_scan(hdr[:-1]) == len(hdr) - 1       # the last header line without its '\n'
    assert lib.sam_header_scan(b"") == 0


def test_records_to_sam_matches_python_writer():
    ann = synth.Annotation("G", n_genes=300, n_refs=3)
    names = ann.as_dict()["refnames"]
    b = ann.reads(1500, "pe", with_records=1, xs_tag=True)
    stream = framed_stream(b, unmapped_every=13)
    got = synth.records_to_sam(stream, names)
    assert got.count(b"\n") > 3000
    assert got == records_to_sam_py(stream, names)


def test_encoder_normalises_synthetic_records():
    """The encoder's view of the writer's text is the synthetic stream with minimal integer tag types and bin recomputed."""
    ann = synth.Annotation("G", n_genes=200, n_refs=2)
    names = ann.as_dict()["refnames"]
    b = ann.reads(400, "pe", with_records=1, xs_tag=True)
    stream = framed_stream(b)
    _, _, every = encode_sam(synth.records_to_sam(stream, names), names)
    # the records agree on everything in front of the tags except bin (and the tags' integer types)
    s1, s2 = bytes(stream), bytes(every)
    p1 = p2 = n = 0
    while p1 < len(s1):
        b1, b2 = struct.unpack_from("<I", s1, p1)[0], struct.unpack_from("<I", s2, p2)[0]
        r1, r2 = s1[p1 + 4:p1 + 4 + b1], s2[p2 + 4:p2 + 4 + b2]
        assert r1[:10] == r2[:10] and r1[12:32] == r2[12:32]
        lqn, ncig, l_seq = r1[8], struct.unpack_from("<H", r1, 12)[0], struct.unpack_from("<I", r1, 16)[0]
        fixed = 32 + lqn + 4 * ncig + (l_seq + 1) // 2
        assert r1[32:fixed] == r2[32:fixed]
        p1 += 4 + b1
        p2 += 4 + b2
        n += 1
    assert p2 == len(s2) and n > 700

"""Generated inputs for the SAM text reader (sam_kernels.hip: k_sam_measure, k_sam_emit; sam_reader.cpp) and the references
they are judged by.  No GPU and no test functions here: tests/test_sam_cases_cpu.py checks the generators and references on
the CPU, tests/test_gpu_sam_fuzz.py runs them through lib.SamReader.

  float literals     float_families / float_text: the expected bits are Python's float() (correctly rounded, as strtod), or
                     float.fromhex, cast to float32 by numpy -- (float)strtod(text), two roundings.  on_fast_path restates the
                     condition in fast_float's comment and only judges the mix of the list.
  valid lines        valid_text: a seeded line grammar; the expected records are tests/test_sam_cpu.py::encode_sam.  coverage()
                     reads the text back and says which of the required cases it holds; missing_coverage() lists the
                     ones it does not.
  malformed lines    malformed_cases: one broken rule on one line of a valid block; first_error is a validator written from
                     the rule comments of sam_kernels.hip with regular expressions and int(), not from the kernels' code.

Left out on purpose: the spelling "-0" of an i tag (and "-00", ...).  The kernels store it as type C; whether htslib stores it
as c or C has not been checked against htslib here, so no generated line holds it and no byte comparison depends on it."""
import decimal
import re
import struct
from collections import Counter, OrderedDict

import numpy as np

# ---- floats -----------------------------------------------------------------------------------------------------------------
_DEC = re.compile(r"^[+-]?(\d*)(?:\.(\d*))?(?:[eE]([+-]?\d+))?$")


def on_fast_path(t):
    """fast_float's comment, restated: [+-]digits[.digits][(e|E)[+-]digits] with at most 19 significant digits, a decimal
    mantissa <= 2^53 and a power of ten within 10^+-22 (a zero mantissa is on the path whatever its exponent)."""
    m = _DEC.match(t)
    if not m or not ((m.group(1) or "") + (m.group(2) or "")):
        return False
    digits = ((m.group(1) or "") + (m.group(2) or "")).lstrip("0")
    if not digits:
        return True
    power = int(m.group(3) or 0) - len(m.group(2) or "")
    return len(digits) <= 19 and int(digits) <= 2 ** 53 and -22 <= power <= 22


def float_ref_bits(texts):
    """uint32 bit patterns of (float)strtod(text) for every text"""
    d = np.array([float.fromhex(t) if "x" in t.lower() else float(t) for t in texts], dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return d.astype(np.float32).view(np.uint32)


def _f32(bits):
    return float(np.array([bits], dtype=np.uint32).view(np.float32)[0])


def _move_point(m, p):
    """spellings of the integer m times 10^p: the exponent explicit, the decimal point moved, and purely positional"""
    s = str(m)
    out = ["%se%d" % (s, p), "%sE%+d" % (s, p)]
    if p == 0:
        out.append(s)
    for k in (1, len(s) - 1):
        out.append("%s.%se%d" % (s[:-k], s[-k:], p + k))
    if p < 0:
        out.append("0." + "0" * (-p - len(s)) + s if -p >= len(s) else s[:p] + "." + s[p:])
    else:
        out.append(s + "0" * p)
    return out


def _midpoints():
    """exact decimal midpoints of adjacent float32 pairs near 1, near 2^-126 and near FLT_MAX, and +-1 in their last place"""
    out = []
    with decimal.localcontext() as c:
        c.prec = 2000
        for base in (0x3f800000, 0x00800000, 0x7f7ffffe):
            for b in range(base - 2, base + 2):
                lo = decimal.Decimal(_f32(b))
                hi = decimal.Decimal(2) ** 128 if b + 1 == 0x7f800000 else decimal.Decimal(_f32(b + 1))
                mid = (lo + hi) / 2
                ulp = decimal.Decimal((0, (1,), mid.as_tuple().exponent))
                for v in (mid, mid + ulp, mid - ulp):
                    for sign in ("", "-"):
                        out.append(sign + "{:e}".format(v))
                    out.append("{:f}".format(v) if base == 0x3f800000 else "{:E}".format(v))
    return out


def float_families(seed=20260):
    """name -> list of literal texts (no tab, no comma)"""
    rng = np.random.RandomState(seed)
    fam = OrderedDict()
    # random finite float32 bit patterns: half over the whole range, half within 2^+-40 (short positional forms)
    n = 11000
    bits = rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32)
    near = (rng.randint(0, 2 ** 32, size=n, dtype=np.uint64).astype(np.uint32) & np.uint32(0x807fffff)) | \
        (rng.randint(127 - 40, 127 + 41, size=n).astype(np.uint32) << np.uint32(23))
    bits = np.concatenate([bits, near])
    bits = bits[(bits >> np.uint32(23)) & np.uint32(0xff) != 0xff]
    vals = [float(v) for v in bits.view(np.float32)]
    for name, f in (("f32 repr", repr), ("f32 %.9g", lambda v: "%.9g" % v), ("f32 %g", lambda v: "%g" % v),
                    ("f32 %e", lambda v: "%e" % v), ("f32 %f", lambda v: "%f" % v), ("f32 %.3f", lambda v: "%.3f" % v)):
        fam[name] = [f(v) for v in vals]
    # random doubles with 15 to 25 significant digits (both sides of the 19-digit limit), some past float32's range
    n = 70000
    x = rng.uniform(1, 10, size=n) * 10.0 ** rng.randint(-48, 41, size=n) * rng.choice([-1.0, 1.0], size=n)
    nd = rng.randint(15, 26, size=n)
    up = rng.randint(0, 2, size=n)
    fam["double 15-25 digits"] = [("%.*E" if u else "%.*e") % (int(d) - 1, float(v)) for v, d, u in zip(x, nd, up)]
    # the mantissa limits at the limits of the power of ten
    lim = []
    for m in (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 10 ** 19 - 1, 10 ** 19, 12345678901234567890):
        for p in (-23, -22, -1, 0, 22, 23):
            lim += _move_point(m, p)
    lim += ["9007199254740992e22", "9.007199254740992e37", "0.0000000000000000000001", "0.00000000000000000000001", "1e22", "1e23",
            "1e-22", "1e-23", "9007199254740993", "9007199254740991e-22"]
    fam["mantissa and power limits"] = lim + ["-" + t for t in lim]
    # ties and double rounding
    tie = []
    for v in list(range(2 ** 24 - 1, 2 ** 24 + 4)) + [(2 ** 24 + 1) << k for k in range(1, 6)] + [(2 ** 24 + 3) << k for k in range(1, 6)]:
        s = str(v)
        tie += [s, "%s.%se%d" % (s[0], s[1:], len(s) - 1), s + "000e-3", "-" + s]
    tie += _midpoints()
    tie += ["3.4028235677973366e38", "3.4028235677973365e38", "-3.4028235677973366e38", "1e-45", "7e-46", "7.1e-46", "1.4e-45",
            "7.006492321624085e-46", "7.006492321624086e-46", "1.0000000596046448", "1.0000000596046447", "1.00000005960464477539062500001"]
    fam["ties and double rounding"] = tie
    fam["spelling"] = ["000.000100", "+.5", "5.", ".5e1", "-0.0", "-0", "0e999999999", "1e-999999", "1e1000000", "-1e1000000",
                       "1E+0000000000000000000022", "1e+0000000000000000000023", "1.5E3", "1.5e3", "1.5E-3", "0.", ".0", "+0", "00012",
                       "0.000000000000000000000000000000000000001e39", "100000000000000000000000000000e-29", "0e-999999999", "1e100000",
                       "1e99999", "1e-100000", "00000000000000000000001", "0.00000000000000000000000000001234567890123456789"]
    fam["host only"] = ["inf", "-Infinity", "NaN", "-nan", " 1.5", "0x1p-149", "0x1.fffffep127", "0x1.ffffffp127", "0X10", "+INF", "nan",
                        "infinity", "0x.8", "0x1.8p1", "-0x1p-150", "0x1.000001p-126", "  -2.5e3"]
    return fam


FLOAT_LINE = "%s\t0\tchr1\t%d\t60\t1M\t*\t0\t0\t*\t*"
FLOAT_HEADER = "@SQ\tSN:chr1\tLN:100000\n"


def float_text(fam, per_array=1500, per_line=200, tail=24000):
    """-> (SAM text, the literals in the order the record stream holds their values).  The hand families go in twice, as B:f
    elements and as single f tags; of the generated ones the last `tail` are f tags (per_line a line), the rest B:f arrays."""
    hand = [t for k, v in fam.items() if not (k.startswith("f32") or k.startswith("double")) for t in v]
    gen = [t for k, v in fam.items() if k.startswith("f32") or k.startswith("double") for t in v]
    rng = np.random.RandomState(7)
    gen = [gen[i] for i in rng.permutation(len(gen))]
    arrays, singles = hand + gen[:-tail], hand + gen[-tail:]
    lines, order = [], []
    for a in range(0, len(arrays), per_array):
        part = arrays[a:a + per_array]
        lines.append(FLOAT_LINE % ("a%d" % a, 10 + len(lines)) + "\tXb:B:f," + ",".join(part))
        order += part
    for a in range(0, len(singles), per_line):
        part = singles[a:a + per_line]
        lines.append(FLOAT_LINE % ("s%d" % a, 10 + len(lines)) + "".join("\tf%s:f:%s" % ("0123456789abcdefghijklmnopqrstuvwxyz"[k % 36], t)
                                                                        for k, t in enumerate(part)))
        order += part
    return ("\n".join(lines) + "\n").encode(), order


def off_path_literals(n, seed):
    """n literals of 20 significant digits: never on the device's path"""
    rng = np.random.RandomState(seed)
    x = rng.uniform(1, 10, size=n) * 10.0 ** rng.randint(-30, 30, size=n)
    out = ["%.19e" % float(v) for v in x]
    assert not any(on_fast_path(t) for t in out)
    return out


def records(stream):
    """the records of a [block_size][record]... stream, without their block_size"""
    s, p, out = bytes(stream), 0, []
    while p < len(s):
        bs = struct.unpack_from("<I", s, p)[0]
        out.append(s[p + 4:p + 4 + bs])
        p += 4 + bs
    assert p == len(s)
    return out


def float_bits(stream):
    """the bit patterns of every f tag and B:f element of a record stream, in stream order (whole arrays and whole runs of f
    tags at a time)"""
    out = []
    for r in records(stream):
        lqn, ncig, l_seq = r[8], struct.unpack_from("<H", r, 12)[0], struct.unpack_from("<I", r, 16)[0]
        q = 32 + lqn + 4 * ncig + (l_seq + 1) // 2 + l_seq
        while q < len(r):
            ty = r[q + 2:q + 3]
            if ty == b"f":
                rest = np.frombuffer(r, dtype=np.uint8, offset=q)
                if rest.size % 7 == 0 and (rest.reshape(-1, 7)[:, 2] == ord("f")).all():   # f tags to the record's end
                    out.append(np.ascontiguousarray(rest.reshape(-1, 7)[:, 3:]).view("<u4").ravel())
                    break
                out.append(np.frombuffer(r, dtype="<u4", count=1, offset=q + 3))
                q += 7
            elif ty == b"B":
                sub, cnt = r[q + 3:q + 4], struct.unpack_from("<I", r, q + 4)[0]
                es = {b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4}[sub]
                if sub == b"f":
                    out.append(np.frombuffer(r, dtype="<u4", count=cnt, offset=q + 8))
                q += 8 + es * cnt
            elif ty in (b"Z", b"H"):
                q = r.index(b"\0", q + 3) + 1
            else:
                q += 3 + {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4}[ty]
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def float_mismatches(got, want, texts, limit=8):
    """(literal, device bits, reference bits) where the two differ; two NaNs are equal whatever their payload"""
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    assert got.shape == want.shape == (len(texts),), (got.shape, want.shape, len(texts))
    nan = lambda b: (b & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    bad = np.nonzero((got != want) & ~(nan(got) & nan(want)))[0]
    return [(texts[i], "0x%08x" % got[i], "0x%08x" % want[i]) for i in bad[:limit]], int(bad.size)


# ---- valid lines ------------------------------------------------------------------------------------------------------------
N_REFS = 1000
OPS = b"MIDNSHP=X"
QUERY_OPS, REF_OPS = b"MIS=X", b"MDN=X"
I_BOUNDS = [-2 ** 31, -2 ** 31 + 1, -32769, -32768, -129, -128, -1, 0, 1, 127, 128, 255, 256, 32767, 32768, 65535, 65536, 2 ** 31 - 1, 2 ** 31,
            2 ** 32 - 1]
B_LIMITS = {b"c": (-128, 127), b"C": (0, 255), b"s": (-32768, 32767), b"S": (0, 65535), b"i": (-2 ** 31, 2 ** 31 - 1), b"I": (0, 2 ** 32 - 1)}
Z_LENS = (0, 1, 127, 128, 129, 5000)
TAG_COUNTS = (0, 1, 63, 64, 65, 200)
OP_COUNTS = (1, 63, 64, 65, 300, 65535, 65536)


def fnv1a(name):
    h = 1469598103934665603
    for c in name:
        h = ((h ^ c) * 1099511628211) & (2 ** 64 - 1)
    return h


def table_slots(names):
    """the open-addressing table sam_reader.cpp describes (FNV-1a, the smallest power of two >= 2 * names + 2, linear probing):
    -> (home slot, final slot) of every name, and the table's size"""
    sz = 2
    while sz < 2 * len(names) + 2:
        sz <<= 1
    used, out = {}, []
    for n in names:
        home = k = fnv1a(n) & 0xffffffff & (sz - 1)
        while k in used and used[k] != n:
            k = (k + 1) & (sz - 1)
        used.setdefault(k, n)
        out.append((home, k))
    return out, sz


def ref_names(seed=5):
    """N_REFS names: prefixes of one another, one-character names, one of 200 characters, and enough whose hash lands on the
    table's last slots that probing wraps to its start"""
    rng = np.random.RandomState(seed)
    names = [b"chr1", b"chr10", b"chr100", b"chr1000", b"chr", b"c", b"1", b"X", b"Y", b"M", b"=x", b"HLA-A*01:01", b"n" * 200,
             b"n" * 199, b"chr1_KI270706v1_random"]
    sz = 2
    while sz < 2 * N_REFS + 2:
        sz <<= 1
    k = 0
    tail = []
    while len(tail) < 6:   # six names whose home is one of the last two slots: at least four of them move, and wrap
        n = b"wrap%d" % k
        k += 1
        if fnv1a(n) & 0xffffffff & (sz - 1) >= sz - 2:
            tail.append(n)
    names += tail
    while len(names) < N_REFS:
        n = bytes(rng.randint(33, 127, size=rng.randint(2, 24)).astype(np.uint8)).replace(b"*", b"s").replace(b"=", b"e")
        if n not in names and not n.startswith(b"@"):
            names.append(n)
    return names


def header_of(names):
    return b"@HD\tVN:1.6\n" + b"".join(b"@SQ\tSN:%s\tLN:%d\n" % (n, 2 ** 31 - 1) for n in names)


SEQ_POOLS = {"plain": b"ACGT", "lower": b"acgtn", "iupac": b"MRSVWYHKDBNmrsvwyhkdbnUu", "eq": b"=ACGT", "digit": b"0123ACGT", "high": bytes(range(128, 256)),
             "any": bytes(c for c in range(33, 127) if c != ord("*"))}


def _bytes_from(rng, pool, n):
    return bytes(np.frombuffer(pool, dtype=np.uint8)[rng.randint(0, len(pool), size=n)])


def _qual(rng, n):
    q = bytes(rng.randint(33, 127, size=n).astype(np.uint8))
    return b"I" if q == b"*" else q


def _tag_name(rng):
    a = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
    return _bytes_from(rng, a, 1) + _bytes_from(rng, a + b"0123456789", 1)


def _cigar_of_len(rng, n):
    """a CIGAR whose text is exactly n bytes (n >= 2), ops of 1 to 3 digits"""
    out, left = [], n
    while left:
        w = int(rng.randint(2, 5))
        if left <= 4:
            w = left
        elif left - w == 1:
            w -= 1 if w > 2 else -1
        d = w - 1
        out.append(b"%d%c" % (rng.randint(10 ** (d - 1), 10 ** d), OPS[rng.randint(0, 9)]))
        left -= w
    return b"".join(out)


def cigar_lens(cigar):
    if cigar == b"*":
        return 0, 0, 0
    ops = re.findall(rb"(\d+)([MIDNSHP=X])", cigar)
    return (sum(int(n) for n, o in ops if o in QUERY_OPS), sum(int(n) for n, o in ops if o in REF_OPS), len(ops))


def _i_text(rng, v, zeros=0):
    s = b"%d" % abs(v)
    return (b"-" if v < 0 else b"+" if rng.randint(0, 8) == 0 else b"") + b"0" * zeros + s


def _b_tag(rng, sub, n, name=None):
    name = name or _tag_name(rng)
    if sub == b"f":
        vals = [b"%g" % v for v in rng.standard_normal(n)] if n != 1 else [b"1e22"]
    else:
        lo, hi = B_LIMITS[sub]
        vals = [b"%d" % v for v in rng.randint(lo, hi + 1, size=n, dtype=np.int64)]
        if n >= 1:
            vals[0] = b"%d" % lo
        if n >= 2:
            vals[-1], vals[1] = b"%d" % hi, b"000%d" % hi
    return name + b":B:" + sub + b"".join(b"," + v for v in vals)


def _rand_tag(rng):
    k = rng.randint(0, 10)
    name = _tag_name(rng)
    if k < 3:
        return name + b":i:" + _i_text(rng, int(rng.randint(-2 ** 31, 2 ** 32, dtype=np.int64)) >> int(rng.randint(0, 33)) or 1)
    if k == 3:
        return name + b":A:" + _bytes_from(rng, SEQ_POOLS["any"], 1)
    if k == 4:
        return name + b":f:" + [b"0.5", b"-1.25e-3", b"1e-40", b"3.4028235e38", b"1.234567890123456789012345", b"nan", b"16777217"][rng.randint(0, 7)]
    if k < 7:
        return name + b":Z:" + _bytes_from(rng, b" " + SEQ_POOLS["any"], int(rng.randint(0, 40)))
    if k == 7:
        return name + b":H:" + _bytes_from(rng, b"0123456789ABCDEF", 2 * int(rng.randint(0, 20)))
    sub = [b"c", b"C", b"s", b"S", b"i", b"I", b"f"][rng.randint(0, 7)]
    return _b_tag(rng, sub, int(rng.randint(0, 12)), name)


class _Text:
    """the text being built: lines with chosen endings, and filler lines that put the next line at a chosen offset mod 16"""

    def __init__(self, rng, names):
        self.rng, self.names, self.parts, self.n, self.k = rng, names, [], 0, 0

    def add(self, line, eol=None):
        eol = eol if eol is not None else (b"\r\n" if self.rng.randint(0, 6) == 0 else b"\n")
        self.parts.append(line + eol)
        self.n += len(line) + len(eol)

    def fields(self, qname=None, flag=None, rname=None, pos=None, mapq=None, cigar=None, rnext=None, pnext=None, tlen=None, seq=None,
               qual=None, tags=(), pool="plain"):
        rng = self.rng
        self.k += 1
        qname = qname if qname is not None else b"r%d" % self.k
        flag = flag if flag is not None else b"%d" % (int(rng.randint(0, 65536)) & ~4)
        rname = rname if rname is not None else self.names[rng.randint(0, len(self.names))]
        pos = pos if pos is not None else b"%d" % rng.randint(1, 2 ** 29)
        mapq = mapq if mapq is not None else b"%d" % rng.randint(0, 256)
        if cigar is None:
            cigar = b"".join(b"%d%c" % (rng.randint(1, 40), OPS[rng.randint(0, 9)]) for _ in range(rng.randint(1, 9)))
        rnext = rnext if rnext is not None else [b"=", b"*", self.names[rng.randint(0, len(self.names))], b"nowhere"][rng.randint(0, 4)]
        pnext = pnext if pnext is not None else b"%d" % rng.randint(0, 2 ** 29)
        tlen = tlen if tlen is not None else b"%d" % rng.randint(-5000, 5000)
        qlen = cigar_lens(cigar)[0]
        if seq is None:
            seq = b"*" if (cigar != b"*" and (qlen == 0 or qlen > 3000)) else _bytes_from(rng, SEQ_POOLS[pool], qlen if cigar != b"*" else int(rng.randint(1, 30)))
        l_seq = 0 if seq == b"*" else len(seq)
        if qual is None:
            qual = b"*" if l_seq == 0 or rng.randint(0, 5) == 0 else _qual(rng, l_seq)
        return b"\t".join([qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual] + list(tags))

    def at_residue(self, res):
        """a filler line after which the text's length is res mod 16"""
        base = self.fields(qname=b"", cigar=b"3M", seq=b"ACG", qual=b"III", rname=b"chr1", pos=b"7", flag=b"0", mapq=b"1", rnext=b"*",
                           pnext=b"0", tlen=b"0")
        pad = (res - (self.n + len(base) + 2)) % 16   # a name of pad + 1 bytes, and the '\n'
        self.add(b"p" * (pad + 1) + base, b"\n")
        assert self.n % 16 == res


def valid_text(seed=11, n_random=1800):
    """-> (text, names): record lines for header_of(names); the last line has no newline"""
    rng = np.random.RandomState(seed)
    names = ref_names()
    T = _Text(rng, names)
    F = T.fields
    known = [b"chr1", b"chr10", b"chr100", b"chr", b"c", b"n" * 200, b"n" * 199] + [n for n in names if n.startswith(b"wrap")]
    # field limits
    T.add(F(qname=b"q"))
    T.add(F(qname=b"Q" * 254))
    T.add(F(flag=b"0"))
    T.add(F(flag=b"65535"))
    T.add(F(flag=b"000000000000000000000000065531"))
    T.add(F(flag=b"00"))
    T.add(F(pos=b"0", pnext=b"0", mapq=b"0", cigar=b"5M"))
    T.add(F(pos=b"2147483647", pnext=b"2147483647", mapq=b"255", cigar=b"3M"))   # bin: the 16 low bits of reg2bin
    T.add(F(pos=b"2147483647", cigar=b"3M100000N3M", rnext=b"="))
    T.add(F(pos=b"536870912", cigar=b"10M"))
    T.add(F(qname=b"far", pos=b"2147483000", cigar=b"3M", rname=b"chr1"))   # reg2bin = 4681 + 131071: the record holds 4680
    T.add(F(tlen=b"-2147483648"))
    T.add(F(tlen=b"2147483647"))
    T.add(F(tlen=b"+5"))
    T.add(F(tlen=b"-0007", pos=b"0000000000000000000000123", mapq=b"0000000000000000000000000255", pnext=b"00000000000000000000009"))
    for n in known:
        T.add(F(rname=n, rnext=known[rng.randint(0, len(known))]))
    for rn in (b"chr2", b"chr10000", b"n" * 201, b"wrap", b"C", b"*"):
        T.add(F(rname=rn))
    for rx in (b"=", b"*", b"chr100", b"unknownRef"):
        T.add(F(rname=b"chr10", rnext=rx))
        T.add(F(rname=b"*", rnext=rx))
    T.add(F(cigar=b"*"))
    T.add(F(cigar=b"5H", seq=b"*", qual=b"*"))
    T.add(F(cigar=b"0M5M", seq=b"ACGTA"))
    T.add(F(cigar=b"005M", seq=b"ACGTA"))
    T.add(F(cigar=b"1M2I3D4N5S6H7P8=9X"))
    T.add(F(cigar=b"1M", seq=b"A", qual=b"*"))
    T.add(F(cigar=b"4M", seq=b"acgt", qual=b"*"))
    # SEQ alphabets, odd and even lengths, lengths around the 32-base vector path
    for pool in SEQ_POOLS:
        for n in (1, 2, 31, 32, 33, 63, 64, 65, 1023, 1024, 1025, 2049):
            T.add(F(cigar=b"%dM" % n, pool=pool))
    # op lengths of 1 to 9 digits (SEQ '*' for the huge ones); rlen stays below 2^31
    for d in range(1, 10):
        v = min(10 ** d - 1, 2 ** 28 - 1)
        T.add(F(cigar=b"%dM%dN%dS" % (v, 10 ** (d - 1), v), seq=b"*", qual=b"*", pos=b"1"))
    T.add(F(cigar=b"268435455M268435455D268435455N268435455=268435455X268435455I268435455S1M", seq=b"*", qual=b"*"))
    # op counts
    for n in OP_COUNTS:
        cig = b"".join(b"%d%c" % (1 + (k % 3), b"MID"[k % 3]) for k in range(n)) if n < 1000 else (b"1M1I" * (n // 2) + b"2M" * (n % 2))
        T.add(F(cigar=cig, seq=None if n < 1000 else b"*", qual=None if n < 1000 else b"*", tags=[b"NM:i:3", b"zz:Z:after the ops"]))
    # CIGAR texts around one and two windows, at every line start mod 16
    for res in range(16):
        for n in [1000 + (res * 3 + k * 17) % 51 for k in range(3)] + [2030 + (res * 5 + k * 13) % 41 for k in range(3)]:
            T.at_residue(res)
            T.add(F(cigar=_cigar_of_len(rng, n), qname=b"w%d_%d" % (res, n)), b"\n")
    for n in list(range(1000, 1051)) + list(range(2030, 2071)):   # and every length once, wherever the line falls
        T.add(F(cigar=_cigar_of_len(rng, n)))
    # tag counts; tags of 5 to 12 bytes so that their prefixes fall on every side of the 1024-byte windows
    for n in TAG_COUNTS:
        for rep in range(4):
            T.add(F(tags=[_tag_name(rng) + b":Z:" + _bytes_from(rng, SEQ_POOLS["any"], int(rng.randint(0, 8))) for _ in range(n)]))
        T.add(F(tags=[_rand_tag(rng) for _ in range(n)]))
    for res in range(16):
        T.at_residue(res)
        T.add(F(tags=[_tag_name(rng) + [b":i:", b":Z:", b":A:"][k % 3] + [b"%d" % (k * 37), b"x" * (k % 5), b"q"][k % 3] for k in range(330)]), b"\n")
    # Z / H lengths around SAM_ZMAX, in the middle of the tags and as the last tag
    for ty in (b"Z", b"H"):
        pool = b" " + SEQ_POOLS["any"] if ty == b"Z" else b"0123456789abcdefABCDEF"
        for n in Z_LENS + (126, 130, 256, 1024):
            v = _bytes_from(rng, pool, n)
            T.add(F(tags=[b"XA:i:1", b"zv:" + ty + b":" + v, b"XB:i:2"]))
            T.add(F(tags=[b"zv:" + ty + b":" + v]))
        T.add(F(tags=[b"z%d:" % k + ty + b":" + _bytes_from(rng, pool, n) for k, n in enumerate((129, 0, 128, 5000, 127, 1, 300))]))
    T.add(F(tags=[b"XA:A:" + bytes([c]) for c in (33, 42, 58, 64, 126)]))
    # i at every type boundary, with 0 to 30 leading zeros
    T.add(F(tags=[b"i%d:i:%d" % (k % 10, v) for k, v in enumerate(I_BOUNDS)]))
    for z in range(1, 31):
        T.add(F(tags=[b"Xz:i:" + _i_text(rng, v, z) for v in (255, I_BOUNDS[(z * 7) % len(I_BOUNDS)], I_BOUNDS[(z * 3 + 1) % len(I_BOUNDS)])]))
    T.add(F(tags=[b"Xz:i:" + b"0" * 20 + b"255", b"Xy:i:-" + b"0" * 12 + b"2147483648", b"Xx:i:+4294967295", b"Xw:i:" + b"0" * 30, b"Xv:i:+0"]))
    # B arrays: every subtype with 0, 1 and 3000 elements, at the subtype's limits
    for sub in (b"c", b"C", b"s", b"S", b"i", b"I", b"f"):
        T.add(F(tags=[b"Be:B:" + sub, _b_tag(rng, sub, 1), b"Bf:B:" + sub, b"XX:i:5"]))
        T.add(F(tags=[_b_tag(rng, sub, 3000), b"Bz:B:" + sub]))
        T.add(F(tags=[_b_tag(rng, sub, 2), _b_tag(rng, sub, 70)]))
    # random lines, some in read-name groups of two or three, some unmapped
    for _ in range(n_random):
        group = [1, 1, 1, 2, 2, 3][rng.randint(0, 6)]
        qn = _bytes_from(rng, b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789_:/#.", int(rng.randint(1, 40)))
        for _g in range(group):
            kw = {}
            if rng.randint(0, 12) == 0:
                kw["flag"] = b"%d" % (int(rng.randint(0, 65536)) | 4)
            if rng.randint(0, 15) == 0:
                kw["rname"] = [b"*", b"notInHeader"][rng.randint(0, 2)]
            if rng.randint(0, 25) == 0:
                kw["cigar"] = b"*"
            if rng.randint(0, 20) == 0:
                kw["pos"] = b"%d" % rng.randint(0, 2 ** 31)
            pool = list(SEQ_POOLS)[rng.randint(0, len(SEQ_POOLS))] if rng.randint(0, 3) == 0 else "plain"
            T.add(F(qname=qn, pool=pool, tags=[_rand_tag(rng) for _ in range(rng.randint(0, 8))], **kw))
    T.add(F(qname=b"last", cigar=b"4M", seq=b"ACGT", qual=b"IIII", tags=[b"Zl:Z:the last line has no newline"]), b"")
    return b"".join(T.parts), names


def split_lines(text):
    """the record lines of a text, without their line ends"""
    lines = text.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    return [l[:-1] if l.endswith(b"\r") else l for l in lines]


def coverage(text, names):
    """which of the cases named in missing_coverage the text holds: key -> count"""
    cov = Counter()
    known = set(names)
    off = 0
    raw = text.split(b"\n")
    if raw[-1] == b"":
        raw.pop()
    else:
        cov["eol:none"] += 1
    for li, rl in enumerate(raw):
        ls = off
        off += len(rl) + 1
        if li < len(raw) - 1 or text.endswith(b"\n"):
            cov["eol:crlf" if rl.endswith(b"\r") else "eol:lf"] += 1
        line = rl[:-1] if rl.endswith(b"\r") else rl
        cov["start:%d" % (ls % 16)] += 1
        f = line.split(b"\t")
        qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
        tags = f[11:]
        if len(qname) in (1, 254):
            cov["qname:%d" % len(qname)] += 1
        if int(flag) in (0, 65535):
            cov["flag:%d" % int(flag)] += 1
        if len(flag) > 1 and flag.startswith(b"0"):
            cov["flag:leading zeros"] += 1
        for nm, v in ((b"pos", pos), (b"pnext", pnext)):
            if int(v) in (0, 2 ** 31 - 1):
                cov["%s:%d" % (nm.decode(), int(v))] += 1
        if int(mapq) in (0, 255):
            cov["mapq:%d" % int(mapq)] += 1
        if int(tlen) in (-2 ** 31, 2 ** 31 - 1):
            cov["tlen:%d" % int(tlen)] += 1
        if tlen == b"+5":
            cov["tlen:+5"] += 1
        cov["rname:" + ("star" if rname == b"*" else "known" if rname in known else "unknown")] += 1
        cov["rnext:" + ("eq" if rnext == b"=" else "star" if rnext == b"*" else "known" if rnext in known else "unknown")] += 1
        if cigar != b"*":
            ops = re.findall(rb"(\d+)([MIDNSHP=X])", cigar)
            for n, o in ops:
                cov["op:" + o.decode()] += 1
                cov["op digits:%d" % len(n)] += 1
                if int(n) == 2 ** 28 - 1:
                    cov["op length:2^28-1"] += 1
            n_ops = len(ops)
            cov["ops:%s" % ("~300" if 250 <= n_ops <= 350 else n_ops)] += 1
            for lo, hi in ((1000, 1050), (2030, 2070)):
                if lo <= len(cigar) <= hi:
                    cov["cigar %d-%d at start %d" % (lo, hi, ls % 16)] += 1
            # where the CIGAR's 1024-byte windows cut it: between two digits of one op, between an op's digits and its letter
            cs = ls + sum(len(x) + 1 for x in f[:5])
            for edge in range((cs & ~15) + 1024, cs + len(cigar), 1024):
                a, b = cigar[edge - cs - 1:edge - cs], cigar[edge - cs:edge - cs + 1]
                cov["cigar window edge:" + ("digit|digit" if a.isdigit() and b.isdigit() else "digit|letter" if a.isdigit() else "letter|digit")] += 1
        if seq == b"*":
            cov["seq:star"] += 1
        else:
            cov["seq:odd" if len(seq) % 2 else "seq:even"] += 1
            for key, pred in (("lower", lambda c: 97 <= c <= 122), ("eq", lambda c: c == 61), ("iupac", lambda c: c in b"MRSVWYHKDB"),
                              ("digit", lambda c: 48 <= c <= 51), ("high", lambda c: c >= 128)):
                if any(pred(c) for c in seq):
                    cov["seq:" + key] += 1
            if any(c >= 128 for c in seq[:len(seq) & ~31]) and len(seq) >= 64:
                cov["seq:high in a vector load"] += 1
            if qual == b"*":
                cov["qual:star with seq"] += 1
                if seq == b"A":
                    cov["seq A qual star"] += 1
        if len(tags) in TAG_COUNTS:
            cov["tags:%d" % len(tags)] += 1
        ts = ls + sum(len(x) + 1 for x in f[:11])
        for t in tags:
            # the prefix XX:T: cut by a window of the measure pass (origin: the line start rounded down to 16) or of the emit pass
            # (origin: the first tag's start rounded down to 16) after 1, 2, 3 or 4 of its bytes
            for nm, org in (("measure", ls & ~15), ("emit", (ls + sum(len(x) + 1 for x in f[:11])) & ~15)):
                cut = 1024 - (ts - org) % 1024
                if 1 <= cut <= 4 and ts - org >= 1024 - 4:
                    cov["tag prefix cut %s:%d" % (nm, cut)] += 1
            ty, val = t[3:4], t[5:]
            if ty in (b"Z", b"H") and len(val) in Z_LENS:
                cov["%s:%d" % (ty.decode(), len(val))] += 1
            if ty == b"A":
                cov["A"] += 1
            if ty == b"i":
                assert int(val) != 0 or not val.startswith(b"-"), "the spelling -0 is left out"
                if int(val) in I_BOUNDS:
                    cov["i:%d" % int(val)] += 1
                z = len(val.lstrip(b"+-")) - len(val.lstrip(b"+-").lstrip(b"0") or b"0")
                if 1 <= z <= 30:
                    cov["i zeros:%d" % z] += 1
                if int(val) == 255 and len(val) == 23:
                    cov["i:255 in 23 digits"] += 1
            if ty == b"B":
                sub = val[:1]
                vals = val[2:].split(b",") if len(val) > 1 else []
                if len(vals) in (0, 1, 3000):
                    cov["B:%s:%d" % (sub.decode(), len(vals))] += 1
                if sub in B_LIMITS:
                    for v in vals:
                        if int(v) in B_LIMITS[sub]:
                            cov["B:%s:%d" % (sub.decode(), int(v))] += 1
            ts += len(t) + 1
    return cov


def missing_coverage(cov):
    """the required cases (every field limit, CIGAR, SEQ and tag shape the GPU test claims to reach) that the text does not hold"""
    need = ["start:%d" % r for r in range(16)] + ["eol:lf", "eol:crlf", "eol:none", "qname:1", "qname:254", "flag:0", "flag:65535",
                                                  "flag:leading zeros", "pos:0", "pos:2147483647", "pnext:0", "pnext:2147483647", "mapq:0", "mapq:255",
                                                  "tlen:-2147483648", "tlen:2147483647", "tlen:+5"]
    need += ["rname:" + x for x in ("known", "unknown", "star")] + ["rnext:" + x for x in ("eq", "star", "known", "unknown")]
    need += ["op:" + chr(c) for c in OPS] + ["op digits:%d" % d for d in range(1, 10)] + ["op length:2^28-1"]
    need += ["ops:%s" % n for n in (1, 63, 64, 65, "~300", 65535, 65536)]
    need += ["cigar %d-%d at start %d" % (lo, hi, r) for lo, hi in ((1000, 1050), (2030, 2070)) for r in range(16)]
    need += ["cigar window edge:" + x for x in ("digit|digit", "digit|letter", "letter|digit")]
    need += ["seq:" + x for x in ("odd", "even", "lower", "eq", "iupac", "digit", "high", "star", "high in a vector load")] + ["qual:star with seq", "seq A qual star"]
    need += ["tags:%d" % n for n in TAG_COUNTS]
    need += ["tag prefix cut %s:%d" % (nm, c) for nm in ("measure", "emit") for c in (1, 2, 3, 4)]
    need += ["%s:%d" % (ty, n) for ty in "ZH" for n in Z_LENS] + ["A"]
    need += ["i:%d" % v for v in I_BOUNDS] + ["i zeros:%d" % z for z in range(1, 31)] + ["i:255 in 23 digits"]
    need += ["B:%s:%d" % (s, n) for s in "cCsSiIf" for n in (0, 1, 3000)]
    need += ["B:%s:%d" % (s.decode(), v) for s, lim in B_LIMITS.items() for v in lim]
    return [k for k in need if cov.get(k, 0) == 0]


# ---- malformed lines --------------------------------------------------------------------------------------------------------
_INT = re.compile(rb"^\d+$")
_SINT = re.compile(rb"^[+-]?\d+$")
_CIGAR = re.compile(rb"^(\d{1,9}[MIDNSHP=X])+$")
_TAG = re.compile(rb"^[A-Za-z][A-Za-z0-9]:(.):", re.S)
# what strtod takes whole (float_syntax's comment): white space, a sign, then a decimal number, a hex number, inf / infinity,
# or nan with an optional (chars)
_FLOAT = re.compile(rb"^[ \v\f\r]*[+-]?(?:(?:\d+\.?\d*|\.\d+)(?:e[+-]?\d+)?|0x(?:[0-9a-f]+\.?[0-9a-f]*|\.[0-9a-f]+)(?:p[+-]?\d+)?|"
                    rb"inf(?:inity)?|nan(?:\([0-9a-z_]*\))?)$", re.I)


def _num(rx, v, lo, hi):
    return bool(rx.match(v)) and lo <= int(v) <= hi


def _tag_rule(t):
    m = _TAG.match(t)
    if not m:
        return "tag"
    ty, v = m.group(1), t[5:]
    if ty == b"A":
        return None if len(v) == 1 else "tag"
    if ty == b"i":
        return "tag" if not _SINT.match(v) else None if -2 ** 31 <= int(v) <= 2 ** 32 - 1 else "out of range"
    if ty == b"f":
        return None if _FLOAT.match(v) else "float"
    if ty in (b"Z", b"H"):
        return None
    if ty == b"B":
        if not v or v[:1] not in b"cCsSiIf" or (len(v) > 1 and v[1:2] != b","):
            return "tag"
        for e in (v[2:].split(b",") if len(v) > 1 else []):
            if v[:1] == b"f":
                if not _FLOAT.match(e):
                    return "float"
            elif not e:
                return "tag"
            else:
                lo, hi = B_LIMITS[v[:1]]
                if not _num(_SINT if lo < 0 else _INT, e, lo, hi):
                    return "out of range"
        return None
    return "tag"


def line_rule(line):
    """the rule a line breaks (None: a valid line), from the rule comments of sam_kernels.hip"""
    if not line:
        return "empty"
    f = line.split(b"\t")
    if len(f) < 11:
        return "fields"
    for t in f[11:]:
        r = _tag_rule(t)
        if r:
            return r
    qname, flag, rname, pos, mapq, cigar, rnext, pnext, tlen, seq, qual = f[:11]
    if cigar != b"*" and not (_CIGAR.match(cigar) and all(int(n) < 2 ** 28 for n in re.findall(rb"\d+", cigar))):
        return "CIGAR"
    if not 1 <= len(qname) <= 254:
        return "QNAME"
    for name, v, rx, lo, hi in (("FLAG", flag, _INT, 0, 65535), ("POS", pos, _INT, 0, 2 ** 31 - 1), ("MAPQ", mapq, _INT, 0, 255),
                                ("PNEXT", pnext, _INT, 0, 2 ** 31 - 1), ("TLEN", tlen, _SINT, -2 ** 31, 2 ** 31 - 1)):
        if not _num(rx, v, lo, hi):
            return name
    qlen, rlen, n_ops = cigar_lens(cigar)
    l_seq = 0 if seq == b"*" else len(seq)
    if n_ops and seq != b"*" and qlen != l_seq:
        return "SEQ length"
    if qual != b"*" and len(qual) != l_seq:
        return "QUAL length"
    if rlen >= 2 ** 31:
        return "too long"
    return None


def first_error(lines):
    """-> (1-based number of the first bad line, the rule it breaks), or None when every line is valid"""
    for k, line in enumerate(lines):
        r = line_rule(line)
        if r:
            return k + 1, r
    return None


BLOCK_REFS = [b"chr1", b"chr2"]
BLOCK_HEADER = b"@SQ\tSN:chr1\tLN:5000000\n@SQ\tSN:chr2\tLN:300000\n"
# the word of .reason that tests/test_gpu_sam.py::test_cli_sam_errors_name_the_line relies on, by the validator's rule
REASON_WORD = {"fields": "fields", "CIGAR": "CIGAR", "float": "float", "out of range": "out of range", "SEQ length": "SEQ length",
               "QUAL length": "QUAL length"}


def valid_block(seed=3, n=50):
    """n valid lines of at most 120 bytes, one read name each, a few of them unmapped"""
    rng = np.random.RandomState(seed)
    T = _Text(rng, BLOCK_REFS)
    out = []
    for k in range(n):
        cig = b"".join(b"%d%c" % (rng.randint(1, 6), b"MIDSX="[rng.randint(0, 6)]) for _ in range(rng.randint(1, 4)))
        tags = [[b"NM:i:%d" % rng.randint(0, 300), b"XS:A:+", b"de:f:0.0123", b"MD:Z:10A5", b"Bc:B:c,-1,2"][j] for j in rng.permutation(5)[:rng.randint(0, 3)]]
        kw = {"flag": b"%d" % (4 if k % 11 == 5 else 16 * (k % 2))}
        out.append(T.fields(qname=b"b%d" % k, cigar=cig, pos=b"%d" % rng.randint(1, 200000), rnext=[b"*", b"=", b"chr2"][k % 3], pnext=b"%d" % rng.randint(0, 9999),
                            tlen=b"%d" % rng.randint(-500, 500), tags=tags, **kw))
        assert len(out[-1]) <= 120
    return out


def _broken(base, field=None, value=None, tag=None):
    f = base.split(b"\t")[:11]
    if field is not None:
        f[field] = value
    return b"\t".join(f + ([tag] if tag is not None else []))


def malformed_cases(seed=3):
    """-> list of (name, lines, 1-based number of the planted line, its rule): a valid block with one rule broken on one line"""
    block = valid_block(seed)
    base = b"bad\t0\tchr1\t100\t60\t4M\t*\t0\t0\tACGT\tIIII"
    star = b"bad\t0\tchr1\t100\t60\t4M\t*\t0\t0\t*\t*"
    plant = [("empty line", b"", "empty"), ("10 fields", b"\t".join(base.split(b"\t")[:10]), "fields"),
             ("QNAME 255", _broken(base, 0, b"q" * 255), "QNAME")]
    plant += [("FLAG " + v.decode(), _broken(base, 1, v), "FLAG") for v in (b"65536", b"-1", b"+1", b"", b"1x", b"1000000000000000000")]
    plant += [("POS 2147483648", _broken(base, 3, b"2147483648"), "POS"), ("MAPQ 256", _broken(base, 4, b"256"), "MAPQ"),
              ("PNEXT -1", _broken(base, 7, b"-1"), "PNEXT"), ("TLEN -2147483649", _broken(base, 8, b"-2147483649"), "TLEN")]
    plant += [("CIGAR " + v.decode(), _broken(star, 5, v), "CIGAR") for v in (b"", b"M", b"5", b"5M3", b"5Q", b"1234567890M", b"268435456M")]
    plant += [("SEQ length", _broken(base, 5, b"5M"), "SEQ length"), ("QUAL length", _broken(base, 10, b"III"), "QUAL length")]
    for t, rule in ((b"X:i:1", "tag"), (b"1X:i:1", "tag"), (b"XX:i", "tag"), (b"XX:q:1", "tag"), (b"XX:A:ab", "tag"), (b"XX:A:", "tag"),
                    (b"XX:i:", "tag"), (b"XX:i:-", "tag"), (b"XX:i:1.0", "tag"), (b"XX:i:4294967296", "out of range"),
                    (b"XX:i:-2147483649", "out of range"), (b"XX:i:" + b"1234567890" * 4, "out of range"), (b"XX:B:x,1", "tag"),
                    (b"XX:B:c1", "tag"), (b"XX:B:c,128", "out of range"), (b"XX:B:C,-1", "out of range"), (b"XX:B:c,,1", "tag"),
                    (b"XX:B:c,1,", "tag"), (b"XX:f:", "float"), (b"XX:f:1e", "float"), (b"XX:f:1.5x", "float"), (b"XX:f:0x", "float"),
                    (b"XX:f:nan(", "float"), (b"XX:f:--1", "float"), (b"XX:B:f,1,,2", "float")):
        plant.append(("tag " + t.decode(), _broken(base, tag=t), rule))
    cases = []
    for k, (name, bad, rule) in enumerate(plant):
        at = 3 + (k * 7) % (len(block) - 6)
        cases.append((name, block[:at] + [bad] + block[at + 1:], at + 1, rule))
    return cases

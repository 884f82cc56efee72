"""A token-level DEFLATE reader written from RFC 1951, and a BGZF walker over it.  No zlib inside: the tests use it to see
what an encoder actually emitted (which block type, which code lengths, which matches at which distance), things that "an
inflater reproduces the input" cannot tell.  No GPU and no test functions here: tests/test_deflate_cases_cpu.py pins it
against zlib-made streams and hand-made bad ones, tests/test_gpu_codec.py reads the device encoder's blocks with it.

It raises DeflateError on what the RFC forbids: an over-subscribed code, an incomplete literal/length or code-length code, an
incomplete distance code other than the single one-bit code (3.2.7: "one distance code of one bit"), a distance beyond the
output so far, a missing end-of-block (the stream ends inside a block, or the code has no symbol 256), a reserved block type
or symbol, a stored block whose NLEN is not ~LEN, and anything but zero padding to the byte after the final block.

Slow (a few hundred KB/s): callers keep what they send through it small."""
import struct

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32     # (30 and 31 never occur in data, 3.2.6; the code is complete with them)


class DeflateError(ValueError):
    pass


def kraft(lens):
    """(numerator of the Kraft sum over 2^15, number of symbols with a code)"""
    return sum(1 << (15 - l) for l in lens if l), sum(1 for l in lens if l)


def check_code(lens, what, one_bit_ok=False, empty_ok=False):
    """The code of these lengths is a complete prefix code; or (distances) empty, or the single one-bit code."""
    if any(l < 0 or l > 15 for l in lens):
        raise DeflateError("%s: a code length beyond 15" % what)
    k, used = kraft(lens)
    if k > 32768:
        raise DeflateError("%s: over-subscribed code (Kraft sum %d / 32768)" % (what, k))
    if used == 0:
        if empty_ok:
            return
        raise DeflateError("%s: no symbol has a code" % what)
    if k < 32768:
        if one_bit_ok and used == 1 and k == 16384:
            return
        raise DeflateError("%s: incomplete code (Kraft sum %d / 32768, %d symbols)" % (what, k, used))


def canonical(lens):
    """3.2.2: {code behind a leading one bit (1 << length | code): symbol}"""
    bl_count = [0] * 16
    for l in lens:
        bl_count[l] += 1
    bl_count[0] = 0
    code, next_code = 0, [0] * 16
    for bits in range(1, 16):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    table = {}
    for sym, l in enumerate(lens):
        if l:
            table[(1 << l) | next_code[l]] = sym
            next_code[l] += 1
    return table


class _Bits:
    def __init__(self, data, pos=0):
        self.data, self.pos = data, pos * 8      # a bit position

    def bits(self, n):
        """n bits, least significant first (data elements other than Huffman codes, 3.1.1)"""
        pos = self.pos
        if pos + n > 8 * len(self.data):
            raise DeflateError("the stream ends inside a block (no end-of-block)")
        self.pos = pos + n
        return (int.from_bytes(self.data[pos >> 3:(pos + n + 7) >> 3], "little") >> (pos & 7)) & ((1 << n) - 1)

    def symbol(self, table, what):
        """Huffman codes come most significant bit first (3.1.1); the key is the code behind a leading one"""
        data, pos, end, key = self.data, self.pos, 8 * len(self.data), 1
        for _ in range(15):
            if pos >= end:
                raise DeflateError("the stream ends inside a block (no end-of-block)")
            key = (key << 1) | ((data[pos >> 3] >> (pos & 7)) & 1)
            pos += 1
            s = table.get(key)
            if s is not None:
                self.pos = pos
                return s
        raise DeflateError("%s: a bit pattern without a symbol (incomplete code)" % what)


class Block:
    """One DEFLATE block: btype, bfinal, hlit / hdist / hclen (the counts, not the header fields: 257.., 1.., 4..) and
    cl_lens (19, in symbol order) / ll_lens / d_lens for btype 2, tokens (an int literal or (length, distance, output
    position)), token_bits (the bit of the stream each token of a coded block starts at), data (the bytes it expands to),
    bit_start / bit_end in the stream."""
    def __init__(self):
        self.btype = self.bfinal = None
        self.hlit = self.hdist = self.hclen = None
        self.cl_lens = self.ll_lens = self.d_lens = None
        self.tokens, self.token_bits, self.data = [], [], b""
        self.bit_start = self.bit_end = 0

    def matches(self):
        return [t for t in self.tokens if not isinstance(t, int)]


def _read_dynamic_header(br, b):
    b.hlit, b.hdist, b.hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise DeflateError("HLIT %d / HDIST %d beyond 286 / 30" % (b.hlit, b.hdist))
    cl = [0] * 19
    for k in range(b.hclen):
        cl[CL_ORDER[k]] = br.bits(3)
    b.cl_lens = cl
    check_code(cl, "code-length code", one_bit_ok=False)
    cl_table = canonical(cl)
    lens = []
    while len(lens) < b.hlit + b.hdist:
        s = br.symbol(cl_table, "code-length code")
        if s < 16:
            lens.append(s)
        elif s == 16:
            if not lens:
                raise DeflateError("repeat of the previous code length at the first one")
            lens += [lens[-1]] * (3 + br.bits(2))
        elif s == 17:
            lens += [0] * (3 + br.bits(3))
        else:
            lens += [0] * (11 + br.bits(7))
    if len(lens) > b.hlit + b.hdist:
        raise DeflateError("a code-length run goes past HLIT + HDIST")
    b.ll_lens, b.d_lens = lens[:b.hlit], lens[b.hlit:]
    check_code(b.ll_lens, "literal/length code")
    check_code(b.d_lens, "distance code", one_bit_ok=True, empty_ok=True)
    if b.ll_lens[256] == 0:
        raise DeflateError("no code for end-of-block")


def inflate(data, start=0, history=b""):
    """All blocks of the raw DEFLATE stream at data[start:]: (blocks, bytes consumed).  Output positions count from the
    first block's first byte; `history` is what a distance may reach before it (none for a BGZF payload)."""
    data = bytes(data)
    br = _Bits(data, start)
    out = bytearray(history)
    h = len(history)
    blocks = []
    fixed_ll, fixed_d = canonical(FIXED_LL), canonical(FIXED_D)
    while True:
        b = Block()
        b.bit_start = br.pos
        b.bfinal, b.btype = br.bits(1), br.bits(2)
        first = len(out)
        if b.btype == 3:
            raise DeflateError("reserved block type 3")
        if b.btype == 0:
            br.pos = (br.pos + 7) & ~7
            n, nn = br.bits(16), br.bits(16)
            if n ^ nn != 0xffff:
                raise DeflateError("stored block: NLEN is not the complement of LEN")
            p = br.pos >> 3
            if p + n > len(data):
                raise DeflateError("the stream ends inside a stored block")
            out += data[p:p + n]
            b.tokens = list(data[p:p + n])
            br.pos += 8 * n
        else:
            if b.btype == 2:
                _read_dynamic_header(br, b)
                ll, dd = canonical(b.ll_lens), canonical(b.d_lens)
            else:
                ll, dd = fixed_ll, fixed_d
            while True:
                t0 = br.pos
                s = br.symbol(ll, "literal/length code")
                if s < 256:
                    out.append(s)
                    b.tokens.append(s)
                    b.token_bits.append(t0)
                elif s == 256:
                    break
                else:
                    if s > 285:
                        raise DeflateError("length symbol %d" % s)
                    length = LEN_BASE[s - 257] + br.bits(LEN_EXTRA[s - 257])
                    if not dd:
                        raise DeflateError("a match in a block without a distance code")
                    d = br.symbol(dd, "distance code")
                    if d > 29:
                        raise DeflateError("distance symbol %d" % d)
                    dist = DIST_BASE[d] + br.bits(DIST_EXTRA[d])
                    if dist > len(out):
                        raise DeflateError("distance %d beyond the %d bytes of output so far" % (dist, len(out)))
                    b.tokens.append((length, dist, len(out) - h))
                    b.token_bits.append(t0)
                    if dist >= length:
                        out += out[len(out) - dist:len(out) - dist + length]
                    else:
                        for _ in range(length):
                            out.append(out[-dist])
        b.data = bytes(out[first:])
        b.bit_end = br.pos
        blocks.append(b)
        if b.bfinal:
            break
    pad = (-br.pos) & 7
    if pad and br.bits(pad) != 0:
        raise DeflateError("non-zero padding after the final block")
    return blocks, (br.pos >> 3) - start


def inflate_exact(payload):
    """The blocks of a payload that must hold one DEFLATE stream and nothing after it."""
    blocks, used = inflate(payload)
    if used != len(payload):
        raise DeflateError("%d bytes after the final block" % (len(payload) - used))
    return blocks


def crc32(data):
    """Bit by bit, the polynomial of RFC 1952 section 8"""
    c = 0xffffffff
    for x in data:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0xEDB88320 if c & 1 else 0)
    return c ^ 0xffffffff


def bgzf_payloads(raw):
    """[(payload, crc32, isize, block size)] of a BGZF byte string (header checked, nothing inflated)"""
    raw = bytes(raw)
    p, out = 0, []
    while p < len(raw):
        if raw[p:p + 4] != b"\x1f\x8b\x08\x04" or raw[p + 10:p + 16] != b"\x06\0BC\x02\0":
            raise DeflateError("no BGZF header at byte %d" % p)
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        if bsize < 26 or p + bsize > len(raw):
            raise DeflateError("BSIZE %d at byte %d" % (bsize, p))
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        out.append((raw[p + 18:p + bsize - 8], crc, isize, bsize))
        p += bsize
    return out


def walk_bgzf(raw):
    """[[Block, ...] per BGZF block]; ISIZE is checked against what the blocks expand to (the CRC is the caller's: zlib's
    is fast, crc32() above is not)."""
    out = []
    for payload, crc, isize, bsize in bgzf_payloads(raw):
        blocks = inflate_exact(payload)
        if sum(len(b.data) for b in blocks) != isize:
            raise DeflateError("ISIZE %d, the blocks expand to %d bytes" % (isize, sum(len(b.data) for b in blocks)))
        out.append(blocks)
    return out

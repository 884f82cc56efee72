"""A token-level DEFLATE / BGZF writer written from RFC 1951 and RFC 1952, the mirror of tests/deflate_ref.py.  No zlib
inside: the tests use it to put in front of the device inflate exactly the stream they mean -- this token with this code at
this bit -- which no encoder can be talked into.  No GPU and no test functions here: tests/inflate_cases.py builds its table
with it, tests/test_inflate_cases_cpu.py pins every stream against zlib and deflate_ref.

A Stream writes stored, fixed and dynamic blocks from explicit tokens (an int literal or (length, distance[, length symbol]))
and keeps the bytes they spell.  Dynamic blocks take explicit code lengths; complete_code() makes a complete code around
prescribed lengths, random_complete_code() one by splitting the Kraft budget at random.  On request it writes wrong things:
raw bits, a bad NLEN, lengths nobody checked, a distance beyond the output, no end-of-block."""
import struct

from tests.deflate_ref import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_D, FIXED_LL, LEN_BASE, LEN_EXTRA, kraft

FULL = 1 << 15      # the Kraft budget of a code of at most 15 bits


class BitWriter:
    def __init__(self):
        self.buf = bytearray()
        self.acc = self.n = 0

    @property
    def pos(self):
        """the bit the next field starts at"""
        return 8 * len(self.buf) + self.n

    def bits(self, v, n):
        """n bits of v, least significant first (3.1.1: everything but Huffman codes)"""
        assert 0 <= v < (1 << n) or n == 0
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 0xff)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """a Huffman code, most significant bit first"""
        self.bits(int(format(code & ((1 << length) - 1), "0%db" % length)[::-1], 2), length)     # (masked: an over-subscribed code runs over)

    def align(self, fill=0):
        if self.n:
            self.bits((1 << (8 - self.n)) - 1 if fill else 0, 8 - self.n)

    def bytes(self, data):
        assert self.n == 0
        self.buf += data

    def getvalue(self, fill=0):
        self.align(fill)
        return bytes(self.buf)


def canonical_codes(lens):
    """3.2.2: [(code, length) or None per symbol]"""
    count = [0] * 17
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for b in range(1, 17):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append((nxt[l], l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def complete_code(n, fixed, fill=None, spread=0, max_len=15):
    """Code lengths of n symbols, complete, in which the symbols of `fixed` ({symbol: length}) have those lengths.  What the
    budget has left goes to the symbols of `fill` (default: the free ones from 0 up), the shortest codes to the first of them;
    spread: use at least that many fill symbols (the shortest code is split in two until there are)."""
    left = FULL - sum(FULL >> l for l in fixed.values())
    assert left >= 0, "the prescribed lengths alone are over-subscribed"
    parts = [1, 1] if left == FULL else [15 - b for b in range(14, -1, -1) if left >> b & 1]     # one code per set bit of what is left
    while len(parts) < spread:
        k = min((i for i, l in enumerate(parts) if l < max_len), key=lambda i: parts[i])
        parts[k] += 1
        parts.insert(k + 1, parts[k])
    fill = [s for s in (range(n) if fill is None else fill) if s not in fixed]
    assert len(parts) <= len(fill) and all(l <= max_len for l in parts), "no room for the rest of the budget"
    lens = [0] * n
    for s, l in fixed.items():
        lens[s] = l
    for s, l in zip(fill, sorted(parts)):
        lens[s] = l
    assert kraft(lens)[0] == FULL
    return lens


def random_complete_code(rng, n, used, must=(), max_len=15, deep=0.5):
    """A complete code over `used` (>= 2) of n symbols, the symbols of `must` among them, made by splitting the Kraft budget: a
    leaf is split in two one bit longer until there are enough; `deep` is how often the split takes the longest leaf."""
    used = max(2, min(used, n), len(must))
    leaves = [1, 1]
    while len(leaves) < used:
        cand = [i for i, l in enumerate(leaves) if l < max_len]
        if rng.rand() < deep:
            top = max(leaves[i] for i in cand)
            cand = [i for i in cand if leaves[i] == top]
        k = cand[rng.randint(len(cand))]
        leaves[k] += 1
        leaves.append(leaves[k])
    rest = [s for s in range(n) if s not in must]
    syms = list(must) + [rest[i] for i in rng.permutation(len(rest))[:used - len(must)]]
    lens = [0] * n
    for s, l in zip(syms, [leaves[i] for i in rng.permutation(used)]):
        lens[s] = l
    assert kraft(lens)[0] == FULL
    return lens


def length_symbol(length, sym=None):
    """(symbol, extra bits' value, their count) of a match length; sym: this symbol and no other (258 = 284 + 31)"""
    if sym is None:
        sym = 285 if length == 258 else max(s for s in range(257, 285) if LEN_BASE[s - 257] <= length)
    x = length - LEN_BASE[sym - 257]
    assert 0 <= x < (1 << LEN_EXTRA[sym - 257]) or x == 0, (length, sym)
    return sym, x, LEN_EXTRA[sym - 257]


def distance_symbol(dist):
    assert 1 <= dist <= 32768, dist
    sym = max(s for s in range(30) if DIST_BASE[s] <= dist)
    return sym, dist - DIST_BASE[sym], DIST_EXTRA[sym]


def rle_ops(lens, runs=True):
    """The code-length section of these lengths as operations: ("len", l), (16, repeat), (17, repeat), (18, repeat);
    runs=False: one ("len", l) per symbol."""
    ops, i = [], 0
    while i < len(lens):
        l, j = lens[i], i
        while j < len(lens) and lens[j] == l:
            j += 1
        run = j - i
        if not runs:
            ops += [("len", l)] * run
        elif l == 0:
            while run >= 11:
                ops.append((18, min(run, 138))); run -= min(run, 138)
            if run >= 3:
                ops.append((17, run)); run = 0
            ops += [("len", 0)] * run
        else:
            ops.append(("len", l)); run -= 1
            while run >= 3:
                ops.append((16, min(run, 6))); run -= min(run, 6)
            ops += [("len", l)] * run
        i = j
    return ops


def ops_lengths(ops):
    """the lengths a list of operations spells"""
    out = []
    for op, v in ops:
        out += [v] if op == "len" else [out[-1]] * v if op == 16 else [0] * v
    return out


def balanced_cl_lens(used, max_len=7):
    """A complete code-length code over the symbols `used` (one more is added if there is only one), as even as it gets."""
    used = sorted(set(used))
    if len(used) == 1:
        used.append(0 if used[0] else 1)
    k = (len(used) - 1).bit_length()
    short = (1 << k) - len(used)
    assert k <= max_len
    lens = [0] * 19
    for i, s in enumerate(used):
        lens[s] = k - 1 if i < short else k
    return lens


class Stream:
    """One raw DEFLATE stream in the making: w (the bits), out (the bytes the tokens spell so far), ll / dd (the open block's
    codes)."""
    def __init__(self):
        self.w = BitWriter()
        self.out = bytearray()
        self.ll = self.dd = None

    # ---- blocks
    def header(self, final, btype):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(btype, 2)

    def stored(self, data, final=False, nlen=None, pad=0):
        self.header(final, 0)
        self.w.align(pad)
        self.w.bits(len(data), 16)
        self.w.bits((len(data) ^ 0xffff) if nlen is None else nlen, 16)
        self.w.bytes(data)
        self.out += data

    def fixed(self, final=False):
        self.header(final, 1)
        self.ll, self.dd = canonical_codes(FIXED_LL), canonical_codes(FIXED_D)
        self.ll_lens, self.d_lens = FIXED_LL, FIXED_D

    def dynamic(self, ll_lens, d_lens, final=False, ops=None, runs=True, cl_lens=None, hclen=None, hlit=None, hdist=None, check=True):
        """The header of a dynamic block.  ops: the code-length section as rle_ops() gives it (default: rle_ops of the lengths,
        with or without runs); cl_lens: the 19 lengths of the code-length code (default: balanced over the symbols the
        operations use); hclen / hlit / hdist: the counts (not the fields), default what the lengths need.  check=False:
        nothing is verified, whatever is asked for is written."""
        ll_lens, d_lens = list(ll_lens), list(d_lens)
        hlit = len(ll_lens) if hlit is None else hlit
        hdist = len(d_lens) if hdist is None else hdist
        if ops is None:
            ops = rle_ops(ll_lens + d_lens, runs)
        if cl_lens is None:
            cl_lens = balanced_cl_lens([v if op == "len" else op for op, v in ops])
        need = max(k for k in range(19) if cl_lens[CL_ORDER[k]]) + 1
        hclen = max(need, 4) if hclen is None else hclen
        if check:
            assert 257 <= hlit <= 286 and 1 <= hdist <= 30 and max(need, 4) <= hclen <= 19
            assert ops_lengths(ops) == ll_lens + d_lens and kraft(cl_lens)[0] == FULL and max(cl_lens) <= 7
            assert kraft(ll_lens)[0] == FULL and ll_lens[256]
            assert kraft(d_lens)[0] == FULL or kraft(d_lens) in ((FULL // 2, 1), (0, 0))
        self.header(final, 2)
        self.w.bits(hlit - 257, 5); self.w.bits(hdist - 1, 5); self.w.bits(hclen - 4, 4)
        for k in range(hclen):
            self.w.bits(cl_lens[CL_ORDER[k]], 3)
        cl = canonical_codes(cl_lens)
        for op, v in ops:
            self.w.code(*cl[v if op == "len" else op])
            if op == 16: self.w.bits(v - 3, 2)
            elif op == 17: self.w.bits(v - 3, 3)
            elif op == 18: self.w.bits(v - 11, 7)
        self.ll, self.dd = canonical_codes(ll_lens + [0] * (288 - len(ll_lens))), canonical_codes(d_lens + [0] * (32 - len(d_lens)))
        self.ll_lens, self.d_lens = ll_lens, d_lens

    # ---- tokens
    def lit(self, b):
        self.w.code(*self.ll[b])
        self.out.append(b)

    def lits(self, data):
        for b in data:
            self.lit(b)

    def match(self, length, dist, sym=None, check=True):
        """check=False: a distance beyond the output is written as it is (the bytes it spells count as zeros)"""
        s, x, n = length_symbol(length, sym)
        self.w.code(*self.ll[s]); self.w.bits(x, n)
        s, x, n = distance_symbol(dist)
        self.w.code(*self.dd[s]); self.w.bits(x, n)
        if check:
            assert dist <= len(self.out), (dist, len(self.out))
        for _ in range(length):
            self.out.append(self.out[-dist] if dist <= len(self.out) else 0)

    def symbol(self, s, distance=False):
        """one bare symbol of the block's code (286, 287, 30, 31: what no token holds)"""
        self.w.code(*(self.dd if distance else self.ll)[s])

    def tokens(self, toks):
        for t in toks:
            if isinstance(t, int): self.lit(t)
            else: self.match(*t)

    def end(self):
        self.w.code(*self.ll[256])

    def raw(self, v, n):
        self.w.bits(v, n)

    def token_bits(self, length, dist, sym=None):
        """how many bits this match takes in the open block's code"""
        s, _, n = length_symbol(length, sym)
        d, _, m = distance_symbol(dist)
        return self.ll[s][1] + n + self.dd[d][1] + m

    def pad_to(self, bit, literals):
        """Spend literals (of `literals`, {byte: its code's length in the open block}) so that the next token starts at `bit`
        of the stream: the longest code while there is room, then whatever sum of the others lands there."""
        gap = bit - self.w.pos
        assert gap >= 0, "already behind bit %d" % bit
        by_len = {}
        for b, l in literals.items():
            assert self.ll[b][1] == l
            by_len.setdefault(l, []).append(b)
        coins = sorted(by_len)
        k = 0
        while gap - coins[-1] >= 4 * coins[-1]:
            b = by_len[coins[-1]]
            self.lit(b[k % len(b)]); k += 1
            gap -= coins[-1]
        how = {0: []}                                 # the rest: a sum of code lengths, fewest literals first
        for g in range(1, gap + 1):
            best = min((how[g - c] + [c] for c in coins if g - c in how), key=len, default=None)
            if best is not None:
                how[g] = best
        assert gap in how, "no sum of %s makes %d bits" % (coins, gap)
        for c in how[gap]:
            b = by_len[c]
            self.lit(b[k % len(b)]); k += 1
        assert self.w.pos == bit

    def finish(self, fill=0):
        return self.w.getvalue(fill)


# ---- BGZF (RFC 1952 with the BC subfield of the SAM specification)
def subfield(si, data):
    return bytes(si) + struct.pack("<H", len(data)) + bytes(data)


def bgzf_frame(payload, data, crc=None, isize=None, before=b"", after=b""):
    """One BGZF block around a payload that spells `data`.  crc / isize: written instead of data's own; before / after: gzip
    extra subfields (subfield()) in front of and behind BC."""
    xlen = len(before) + 6 + len(after)
    bsize = 12 + xlen + len(payload) + 8
    assert bsize <= 65536, "a BGZF block holds 64 KiB, this one has %d bytes" % bsize
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff" + struct.pack("<H", xlen) + before + b"BC\x02\0" + struct.pack("<H", bsize - 1) + after + payload
            + struct.pack("<II", crc32_fast(data) if crc is None else crc, len(data) if isize is None else isize))


_CRC_TABLE = []


def crc32_fast(data):
    """deflate_ref.crc32 a byte at a time, through the table of RFC 1952 section 8 (checked against it in the CPU tests)"""
    if not _CRC_TABLE:
        for i in range(256):
            v = i
            for _ in range(8):
                v = (v >> 1) ^ (0xEDB88320 if v & 1 else 0)
            _CRC_TABLE.append(v)
    c = 0xffffffff
    for x in bytes(data):
        c = _CRC_TABLE[(c ^ x) & 0xff] ^ (c >> 8)
    return c ^ 0xffffffff

"""The named streams tests/test_gpu_inflate_crafted.py puts in front of k_inflate, built token by token with
tests/deflate_write.py.  No GPU and no test functions here: tests/test_inflate_cases_cpu.py checks every one of them against
zlib and tests/deflate_ref.py, and that each is what its name says (Case.claim, asserted from deflate_ref's Block objects).

Classes.  valid: zlib inflates the payload to exactly `want`, the device must too.  invalid: zlib raises or the result
disagrees with the frame's ISIZE / CRC32, the device must refuse (`note`: the line of k_inflate that does, found by reading
it; every one is a `bad = true` with no access behind it).  lenient: zlib raises for a reason the kernel's header comment
lets pass (an incomplete code nobody uses the holes of, non-zero padding, bytes behind the final block); the device refuses
or returns exactly `want`.

The kernel's geometry the cases aim at (inflate_kernels.hip): a 1 KiB input ring refilled in 512-byte chunks (a chunk edge every
4096 bits, the ring's wrap every 8192), a 64-bit decode buffer (lane i decodes the token at bit i; a step takes the literals and
the short matches -- at most 32 bytes, distance code at most 8 bits -- on the chain from bit 0 up to the first token that is
neither), a 2 KiB output window flushed in 512-byte pieces; a match reads the window when dist + (hi - at) <= 2048 (hi: the end
of what the step writes) and the wave's own output in HBM otherwise."""
import functools
import os
import struct
import zlib

import numpy as np

from tests import deflate_ref as R
from tests import deflate_write as W

OUT_WIN, OUT_PIECE, CHUNK_BITS, D_BITS, SHORT = 2048, 512, 4096, 8, 32


class Case:
    """name, cls (valid / invalid / lenient), payload (raw DEFLATE), want (the bytes the tokens spell: for an invalid case
    only what its frame is made from), crc / isize / clen (what the frame or the table entry says), raw (the BGZF block;
    None: the payload does not fit one, or the entry says what no frame can, and it goes in by a hand-made table entry), claim (blocks -> None, asserts what the name says), note (invalid: the refusing line),
    why (invalid / lenient: a piece of deflate_ref's message, or "isize" / "crc" / "short" where the stream itself is fine)"""
    def __init__(self, name, cls, payload, want, claim=None, note="", why="", crc=None, isize=None, framed=True, before=b"", after=b"", clen=None):
        self.name, self.cls, self.payload, self.want, self.claim, self.note, self.why = name, cls, bytes(payload), bytes(want), claim, note, why
        self.crc = W.crc32_fast(self.want) if crc is None else crc
        self.isize = len(self.want) if isize is None else isize
        self.clen = len(self.payload) if clen is None else clen
        self.raw = W.bgzf_frame(self.payload, b"", self.crc, self.isize, before, after) if framed else None
        self.xlen = 6 + len(before) + len(after)

    @property
    def expected(self):
        """the bytes the device must return; None: it must refuse"""
        return None if self.cls == "invalid" else self.want

    def direct(self):
        """the bytes behind a hand-made table entry (src_off: their first, clen, ulen = isize, crc): the payload and eight more"""
        return self.payload + struct.pack("<II", self.crc, self.isize)


def zlib_inflate(payload):
    """(bytes, reached the end of the stream, bytes left over); zlib.error goes up"""
    d = zlib.decompressobj(-15)
    out = d.decompress(payload)
    return out, d.eof, d.unused_data


# ---- what the kernel will do with a block's tokens: its steps ---------------------------------------------------------------
def steps(b):
    """The decode steps of a coded block as k_inflate takes them: [{pos, hi, tokens: [index], term: index or None}].  A step
    starts at a token; tokens that start less than 64 bits behind it join it while they are literals or short matches with a
    distance code of at most D_BITS bits; the first other token ends it (term) and is taken after the step's bytes; a token 64
    bits or more behind starts the next step.  hi: the output position behind the step's own bytes (term's not among them)."""
    out, k, n = [], 0, len(b.tokens)
    # output positions of all tokens: from the first match's own (the block's first byte is 0 if it has none)
    pos_of, run = [], 0
    for t in b.tokens:
        pos_of.append(run)
        run += 1 if isinstance(t, int) else t[0]
    base = 0
    for i, t in enumerate(b.tokens):
        if not isinstance(t, int):
            base = t[2] - pos_of[i]
            break
    while k < n:
        st = {"pos": base + pos_of[k], "tokens": [], "term": None, "bit": b.token_bits[k]}
        while k < n and b.token_bits[k] - st["bit"] < 64:
            t = b.tokens[k]
            if isinstance(t, int) or (t[0] <= SHORT and b.d_lens[W.distance_symbol(t[1])[0]] <= D_BITS):
                st["tokens"].append(k); k += 1
                continue
            st["term"] = k; k += 1
            break
        st["hi"] = st["pos"] + sum(1 if isinstance(b.tokens[i], int) else b.tokens[i][0] for i in st["tokens"])
        out.append(st)
    return out


def step_of(b, index):
    for st in steps(b):
        if index in st["tokens"] or index == st["term"]:
            return st
    raise AssertionError("token %d is in no step" % index)


def find_match(b, length, dist, pos=None):
    hits = [i for i, t in enumerate(b.tokens) if not isinstance(t, int) and t[0] == length and t[1] == dist and (pos is None or t[2] == pos)]
    assert hits, "no match (%d, %d) at %s" % (length, dist, pos)
    return hits[0]


# ---- codes ------------------------------------------------------------------------------------------------------------------
# the probe code: 'A' in one bit, 'B' in two, literals 0 .. 11 in 3 .. 14 bits, end-of-block and length symbol 284 (227 .. 257,
# and 258 as 284 + 31) in 15; distances: 1 and 257 .. 384 in two bits, 16385 .. 32768 (13 extra bits) in 15
LL_PROBE = W.complete_code(286, {65: 1, 66: 2, 256: 15, 284: 15})
D_PROBE = W.complete_code(30, {0: 2, 16: 2, 28: 15, 29: 15}, fill=[8] + list(range(1, 8)) + list(range(9, 16)))
D_PROBE8 = W.complete_code(30, {0: 2, 16: 2, 28: 8, 29: 8}, fill=list(range(1, 16)))     # the same with 8-bit codes for 28 / 29
# the window code: four literals in 2, 2, 3, 3 bits, end-of-block and every length symbol in the quarter that is left
LL_WIN = W.complete_code(286, {97: 2, 98: 2, 99: 3, 100: 3}, fill=list(range(256, 286)), spread=30)
D_FLAT = W.complete_code(30, {}, spread=30)
ABCD = (97, 98, 99, 100)


def probe_stream(d_lens=D_PROBE, room=16600):
    """a dynamic block in the probe code with `room` bytes of output in front of what follows (258 'A's, then copies of them)"""
    s = W.Stream()
    s.dynamic(LL_PROBE, d_lens, final=True)
    s.lits([65, 66] * 129)
    while len(s.out) < room:
        s.match(258, 258, 284)
    return s


def done(s):
    s.end()
    return s.finish()


def widest(s, k):
    """the widest token there is: 15 + 5 + (distance code) + 13 bits, its extra bits varied with k"""
    length = 227 + (k * 7) % 31
    dist = 16385 + (k * 2654435761) % min(16384, len(s.out) - 16384)
    s.match(length, dist, 284)
    return length, dist


# ---- the cases --------------------------------------------------------------------------------------------------------------
def long_code_cases():
    for n in range(11, 16):
        # a literal, a short and a long length, the end-of-block, each in n bits, behind 'A' in one bit
        ll = W.complete_code(286, {65: 1, 200: n, 260: n, 285: n, 256: n})
        s = W.Stream()
        s.dynamic(ll, [1], final=True)
        s.tokens([65, 65, 200, 65, 200, 200, 65, 65, 65, (6, 1), 65, (258, 1), 200, (6, 1), 200])

        def claim(bl, n=n):
            b = bl[0]
            assert [b.ll_lens[x] for x in (200, 260, 285, 256)] == [n] * 4
            assert 200 in b.tokens and (6, 1, 9) in b.tokens and any(not isinstance(t, int) and t[0] == 258 for t in b.tokens)
        yield Case("long codes: literal, lengths and end-of-block in %d bits" % n, "valid", done(s), s.out, claim)
    for n in range(9, 16):
        d = W.complete_code(30, {5: n, 0: 1})
        s = W.Stream()
        s.dynamic(LL_WIN, d, final=True)
        s.lits([97, 98, 99, 100, 97, 97, 98, 100, 99])
        s.tokens([(4, 7), 98, (5, 8), 99, 99, (4, 1), (40, 8), 97])

        def claim(bl, n=n):
            b = bl[0]
            assert b.d_lens[5] == n and (4, 7, 9) in b.tokens and any(not isinstance(t, int) and t[:2] == (40, 8) for t in b.tokens)
        yield Case("long codes: a short match with a distance code of %d bits" % n, "valid", done(s), s.out, claim)


def alphabet_cases():
    for kind in ("fixed", "dynamic"):
        s = W.Stream()
        if kind == "fixed":
            s.fixed(final=True)
        else:
            rng = np.random.RandomState(41)
            s.dynamic(W.random_complete_code(rng, 286, 286, max_len=15, deep=0.6), W.random_complete_code(rng, 30, 30, max_len=15, deep=0.6), final=True)
        s.lits(bytes(range(7, 7 + 200)))
        while len(s.out) < 32768:
            s.match(258, 199 if len(s.out) % 3 else 200)
        for k in range(29):
            for length in (R.LEN_BASE[k], R.LEN_BASE[k] + (1 << R.LEN_EXTRA[k]) - 1):
                s.match(length, 300 + k, 257 + k)
                s.lit(k)
        for k in range(30):
            for dist in (R.DIST_BASE[k], R.DIST_BASE[k] + (1 << R.DIST_EXTRA[k]) - 1):
                s.match(5, dist)
                s.lit(100 + k)

        def claim(bl, kind=kind):
            b = bl[0]
            m = b.matches()
            assert {t[0] for t in m} >= set(R.LEN_BASE) | {R.LEN_BASE[k] + (1 << R.LEN_EXTRA[k]) - 1 for k in range(29)}
            assert {t[1] for t in m} >= set(R.DIST_BASE) | {R.DIST_BASE[k] + (1 << R.DIST_EXTRA[k]) - 1 for k in range(30)}
            assert any(t[1] == 32768 for t in m)
            if kind == "dynamic":
                assert b.hlit == 286 and b.hdist == 30 and all(b.ll_lens) and all(b.d_lens) and max(b.ll_lens) == 15 and max(b.d_lens) == 15
        yield Case("alphabets: every length and distance symbol at its lowest and highest extra bits, distance 32768 (%s)" % kind, "valid", done(s), s.out, claim)

    s = probe_stream(room=300)
    s.match(258, 258, 284); s.match(258, 1, 284); s.lit(66); s.match(258, 2, 284)
    payload = done(s)

    def claim(bl):
        assert bl[0].ll_lens[284] == 15 and bl[0].ll_lens[285] == 0 and sum(1 for t in bl[0].matches() if t[0] == 258) >= 3
    yield Case("alphabets: length 258 as symbol 284 with 31 extra bits", "valid", payload, s.out, claim)

    for sym in (0, 1):
        s = W.Stream()
        s.dynamic(LL_WIN, [0] * sym + [1], final=True)
        s.tokens([97, 98, 99, (3, sym + 1), (32, sym + 1), 100, (258, sym + 1), (33, sym + 1)])

        def claim(bl, sym=sym):
            assert bl[0].d_lens == [0] * sym + [1] and {t[1] for t in bl[0].matches()} == {sym + 1}
        yield Case("alphabets: the single one-bit distance code, symbol %d" % sym, "valid", done(s), s.out, claim)

    s = W.Stream()
    s.dynamic(LL_WIN, [0], final=True)
    s.lits([97, 98, 99, 100] * 40)

    def claim(bl):
        assert bl[0].hdist == 1 and bl[0].d_lens == [0] and not bl[0].matches()
    yield Case("alphabets: HDIST = 1 with a zero length, no distances", "valid", done(s), s.out, claim)

    ll = W.complete_code(286, {97: 1, 256: 2, 285: 3, 284: 3})
    s = W.Stream()
    s.dynamic(ll, [1], final=True)
    s.tokens([97, (258, 1), (257, 1), 97])

    def claim(bl):
        assert bl[0].hlit == 286 and bl[0].ll_lens[285] == 3
    yield Case("alphabets: HLIT = 286", "valid", done(s), s.out, claim)


def code_length_cases():
    # 18 at every repeat count: one tiny block each (literal 0 and end-of-block in one bit, 255 zeros between them)
    for sym, counts in ((18, range(11, 139)), (17, range(3, 11)), (16, range(3, 7))):
        s = W.Stream()
        for rep in counts:
            if sym == 18:
                ll = [1] + [0] * 255 + [1]
                ops = [("len", 1), (18, rep)] + W.rle_ops([0] * (255 - rep) + [1] + [0])
                s.dynamic(ll, [0], ops=ops)
                s.lits([0, 0])
            elif sym == 17:
                ll = W.complete_code(257, {0: 1, rep + 1: 2}, fill=[256] + list(range(200, 256)))
                ops = [("len", 1), (17, rep)] + W.rle_ops(ll[rep + 1:] + [1])
                s.dynamic(ll, [1], ops=ops)
                s.tokens([0, rep + 1, 0])
            else:
                ll = W.complete_code(257, dict([(k, 4) for k in range(rep + 1)] + [(256, 2)]), fill=list(range(100, 256)))
                ops = [("len", 4), (16, rep)] + W.rle_ops(ll[rep + 1:] + [1])
                s.dynamic(ll, [1], ops=ops)
                s.tokens([0, rep, 1])
            s.end()
        s.fixed(final=True)
        s.lit(33)

        def claim(bl, sym=sym, counts=counts):
            assert len(bl) == len(counts) + 1 and all(b.btype == 2 for b in bl[:-1])
            for b, rep in zip(bl, counts):     # the run is there: that many equal lengths behind the first
                want = 0 if sym != 16 else 4
                assert b.ll_lens[1:1 + rep] == [want] * rep and b.cl_lens[sym] > 0
                assert sym != 18 or b.ll_lens[1 + rep:256] == [0] * (255 - rep)
        yield Case("code lengths: symbol %d at every repeat count" % sym, "valid", done(s), s.out, claim)

    # a 16 that starts in the literal/length lengths and ends in the distance lengths
    ll = W.complete_code(286, {284: 5, 285: 5, 97: 1, 256: 3})
    d = W.complete_code(30, {0: 5, 1: 5, 2: 5})
    s = W.Stream()
    s.dynamic(ll, d, final=True, ops=W.rle_ops(ll[:284]) + [("len", 5), (16, 4)] + W.rle_ops(d[3:]))
    s.tokens([97, 97, 97, 97, (258, 1), (258, 2), (257, 3), 97])

    def claim(bl):
        b = bl[0]
        assert b.hlit == 286 and b.ll_lens[284:] == [5, 5] and b.d_lens[:3] == [5, 5, 5] and {t[1] for t in b.matches()} == {1, 2, 3}
    yield Case("code lengths: a symbol-16 run from the literal/length lengths into the distance lengths", "valid", done(s), s.out, claim)

    # code-length codes of up to 7 bits, every length written out (no 16 / 17 / 18), HCLEN 19
    ll = W.complete_code(257, {65: 1, 256: 7})      # literals 0 .. 5 take 2 .. 7 bits
    cl = [1, 2, 3, 4, 5, 6, 7, 7] + [0] * 11
    s = W.Stream()
    s.dynamic(ll, [1], final=True, runs=False, cl_lens=cl, hclen=19)
    s.tokens([65, 0, 1, 2, 3, 4, 5, 65, 5, 0])

    def claim(bl):
        b = bl[0]
        assert b.cl_lens == [1, 2, 3, 4, 5, 6, 7, 7] + [0] * 11 and b.hclen == 19 and sorted(set(b.ll_lens)) == list(range(8))
    yield Case("code lengths: 7-bit code-length codes, no run symbols, HCLEN 19", "valid", done(s), s.out, claim)


def ring_cases():
    """the widest token at every bit from 4096 k - 48 to 4096 k, k = 1, 2, 3 (one stream takes the three k)"""
    for off in range(49):
        s = probe_stream()
        marks = []
        for k in (1, 2, 3):
            s.pad_to(CHUNK_BITS * k - off, {65: 1, 66: 2, 11: 14})
            marks.append((s.w.pos,) + widest(s, off + k))
            s.lits([66, 65, 0, 1])

        def claim(bl, marks=marks, off=off):
            b = bl[0]
            for k, (bit, length, dist) in zip((1, 2, 3), marks):
                i = find_match(b, length, dist)
                assert b.token_bits[i] == bit == CHUNK_BITS * k - off
                assert b.ll_lens[284] == 15 and b.d_lens[W.distance_symbol(dist)[0]] == 15 and W.distance_symbol(dist)[2] == 13
        yield Case("ring sweep: the 48-bit token %d bits in front of bits 4096, 8192 and 12288" % off, "valid", done(s), s.out, claim)


def lane_cases():
    """the widest token behind n one-bit literals, n = 0 .. 70: at every lane of the buffer and behind it"""
    for name, d_lens, bits in (("48-bit token (distance code of 15 bits, taken bit by bit)", D_PROBE, 15), ("41-bit token (distance code of 8 bits, taken by its lane)", D_PROBE8, 8)):
        s = probe_stream(d_lens)
        s.match(258, 258, 284)
        marks = []
        for n in range(71):
            at = s.w.pos
            s.lits([65] * n)
            marks.append((at, n, s.w.pos) + widest(s, n))

        def claim(bl, marks=marks, bits=bits):
            b = bl[0]
            for at, n, bit, length, dist in marks:
                hits = [j for j, t in enumerate(b.tokens) if b.token_bits[j] == bit]
                assert len(hits) == 1 and b.tokens[hits[0]][:2] == (length, dist) and bit - at == n
                j = hits[0]
                assert b.tokens[j - n:j] == [65] * n and not isinstance(b.tokens[j - n - 1], int)     # a long match in front: the step starts at `at`
                assert b.token_bits[j - n] == at and step_of(b, j - n)["bit"] == at
                assert b.ll_lens[284] == 15 and b.d_lens[W.distance_symbol(dist)[0]] == bits and W.distance_symbol(dist)[2] == 13
        yield Case("lane sweep: the " + name + " behind 0 .. 70 one-bit literals", "valid", done(s), s.out, claim)


def window_stream(start, seed):
    """a dynamic block in the window code with `start` bytes of unruly output"""
    rng = np.random.RandomState(seed)
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True)
    s.lits(rng.choice(ABCD, size=300))
    while len(s.out) < start - 2600:
        s.match(258, int(rng.randint(1, min(32768, len(s.out)) + 1)))
    while len(s.out) < start:
        if rng.rand() < 0.5: s.lits(rng.choice(ABCD, size=rng.randint(1, 9)))
        else: s.match(int(rng.randint(3, 60)), int(rng.randint(1, min(32768, len(s.out)) + 1)))
    return s, rng


def other(b):
    return 97 if b != 97 else 98


def window_cases():
    for start in (3000, 40000):
        # short matches inside a step: r literals, the match, t literals, then a long match that ends the step
        s, rng = window_stream(start, start)
        probes = []
        for r in (0, 1, 8):
            for t in (0, 1, 5):
                for length in (3, 17, 32):
                    for d in (-1, 0, 1):
                        dist = OUT_WIN - (length + t) + d
                        s.match(40 + r + t, int(rng.randint(1, 3000)))        # ends the step before
                        s.lits(rng.choice(ABCD, size=r))
                        at = len(s.out)
                        s.match(length, dist)
                        if t:   # the byte that takes the source's place in the window if the far path is missed differs from it
                            s.lits(list(rng.choice(ABCD, size=t - 1)) + [other(s.out[at - dist] if d == 1 else 0)])
                        probes.append((at, length, dist, r, t, d))
        s.match(50, 7)

        def claim(bl, probes=probes, start=start):
            b = bl[0]
            assert start <= probes[0][0] and probes[-1][0] < start + 8000
            for at, length, dist, r, t, d in probes:
                i = find_match(b, length, dist, at)
                st = step_of(b, i)
                assert st["tokens"] == list(range(i - r, i + t + 1)) and st["term"] == i + t + 1, (at, st)
                assert all(isinstance(b.tokens[j], int) for j in st["tokens"] if j != i)
                assert dist + (st["hi"] - at) == OUT_WIN + d and st["hi"] - at == length + t
        yield Case("window sweep: short matches inside a step around output position %d" % start, "valid", done(s), s.out, claim)

        # long matches that end a step, r literals in front of them in it; 2047 / 2048 / 2049; a far source that ends on a piece
        s, rng = window_stream(start, start + 1)
        probes = []
        for r in (0, 5):
            for length in (33, 100, 258):
                for dist in (OUT_WIN - length - 1, OUT_WIN - length, OUT_WIN - length + 1, 2047, 2048, 2049):
                    s.match(35, int(rng.randint(1, 3000)))
                    s.lits(rng.choice(ABCD, size=r))
                    probes.append((len(s.out), length, dist, r))
                    s.match(length, dist)
        s.match(35, 9)
        s.lits([97] * ((-len(s.out)) % OUT_PIECE + 7))
        edge = (len(s.out) - 7 - 5 * OUT_PIECE - 100, 100, len(s.out))      # source [.., a piece's end)
        s.match(edge[1], edge[2] - edge[0])

        def claim(bl, probes=probes, edge=edge):
            b = bl[0]
            for at, length, dist, r in probes:
                i = find_match(b, length, dist, at)
                st = step_of(b, i)
                assert st["term"] == i and st["tokens"] == list(range(i - r, i)) and st["hi"] == at
            i = find_match(b, edge[1], edge[2] - edge[0], edge[2])
            assert (edge[0] + edge[1]) % OUT_PIECE == 0 and edge[2] - edge[0] > OUT_WIN
        yield Case("window sweep: long matches at the window's edge, 2047 / 2048 / 2049, a far source ending on a piece, around %d" % start, "valid", done(s), s.out, claim)


def step_cases():
    s = probe_stream(room=300)
    s.match(258, 258, 284)
    s.lits([65] * 64 + [66] + [65] * 130 + [66, 66] + [65] * 63 + [66])

    def claim(bl):
        b = bl[0]
        i = find_match(b, 258, 258, 516)
        st = step_of(b, i + 1)
        assert b.tokens[i + 1:i + 65] == [65] * 64 and len(st["tokens"]) == 64 and st["term"] is None
    yield Case("steps: 64 one-bit literals in one step", "valid", done(s), s.out, claim)

    # the most a step writes: 16 matches of 32 bytes in four bits each (32 by a one-bit code and two extra bits, a one-bit
    # distance), and 32 matches of 10 bytes in two bits each
    for length, sym, count in ((32, 272, 16), (10, 264, 32)):
        ll = W.complete_code(286, {sym: 1, 97: 2, 285: 4, 256: 4})
        s = W.Stream()
        s.dynamic(ll, [1, 1], final=True)
        s.lits([97, 0, 97])
        s.match(258, 1)
        s.tokens([(length, 1 + k % 2) for k in range(count)] + [(258, 2)] + [(length, 2)] * (count + 3) + [97, (258, 1)])

        def claim(bl, length=length, count=count):
            b = bl[0]
            st = steps(b)[1]
            assert len(st["tokens"]) == count and st["hi"] - st["pos"] == count * length and st["term"] is None      # (64 bits of tokens: the 258 behind them is the next step's)
            assert all(b.tokens[i][0] == length for i in st["tokens"])
        yield Case("steps: %d matches of %d bytes in one step" % (count, length), "valid", done(s), s.out, claim)

    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True)
    rng = np.random.RandomState(8)
    s.lits(rng.choice(ABCD, size=60))
    for dist in (1, 2, 3, 31, 33):
        s.match(40, 50)
        s.lits(rng.choice(ABCD, size=3))
        s.match(32, dist)
        s.match(20, dist)
        s.lit(99)
    # a match that repeats this step's literals, one that repeats that match, one that repeats itself from them
    s.match(40, 50)
    s.tokens([97, 98, 99, (3, 3), (6, 6), (30, 2), 100, (4, 1)])
    at = len(s.out)

    def claim(bl, at=at):
        b = bl[0]
        for dist in (1, 2, 3, 31, 33):
            i = [j for j, t in enumerate(b.tokens) if not isinstance(t, int) and t[:2] == (32, dist)][0]
            assert i in step_of(b, i)["tokens"] and i + 1 in step_of(b, i)["tokens"]
        i = [j for j, t in enumerate(b.tokens) if not isinstance(t, int) and t[:2] == (3, 3)][-1]
        assert step_of(b, i)["tokens"][:8] == list(range(i - 3, i + 5))
    yield Case("steps: overlapping short matches at distances 1, 2, 3, 31, 33; matches that repeat the step's own bytes", "valid", done(s), s.out, claim)

    for name, dists in (("1, 2, 3, 63, 64, 65, 257, 258", (1, 2, 3, 63, 64, 65, 257, 258)),
                        ("where the quotient by reciprocal is one short (41, 47, 55, 61, 83, 97, 141, 249)", (41, 47, 55, 61, 83, 97, 141, 249))):
        s = W.Stream()
        s.fixed(final=True)
        s.lits(np.random.RandomState(9).randint(0, 256, size=270))
        for dist in dists:
            s.match(258, dist)
            s.lits([dist & 255, 3])

        def claim(bl, dists=dists):
            assert [t[:2] for t in bl[0].matches()] == [(258, d) for d in dists]
        yield Case("steps: 258-byte matches at distances " + name, "valid", done(s), s.out, claim)

    for pos in (1, 5000):
        s = W.Stream()
        s.dynamic(LL_WIN, D_FLAT, final=True)
        s.lits(np.random.RandomState(pos).choice(ABCD, size=pos))
        s.match(20, pos); s.match(200, pos + 20)

        def claim(bl, pos=pos):
            assert bl[0].matches() == [(20, pos, pos), (200, pos + 20, pos + 20)]
        yield Case("steps: dist == pos at output position %d" % pos, "valid", done(s), s.out, claim)


def stored_cases():
    rng = np.random.RandomState(12)
    for n in (0, 1):
        s = W.Stream()
        s.fixed(); s.lits(b"xy"); s.end()
        s.stored(bytes(rng.randint(0, 256, size=n).astype(np.uint8)), final=True)

        def claim(bl, n=n):
            assert bl[1].btype == 0 and len(bl[1].data) == n
        yield Case("stored: a block of %d bytes" % n, "valid", s.finish(), s.out, claim)

    s = W.Stream()
    s.stored(bytes(rng.randint(0, 256, size=65535).astype(np.uint8)), final=True)

    def claim(bl):
        assert bl[0].btype == 0 and len(bl[0].data) == 65535
    yield Case("stored: a block of 65535 bytes (no BGZF frame holds it: by a table entry)", "valid", s.finish(), s.out, claim, framed=False)

    # LEN / NLEN across a chunk edge: LEN at byte 511 (its second byte in the next chunk), then NLEN across the next edge
    s = W.Stream()
    s.fixed(); s.lits(rng.randint(0, 144, size=509)); s.end()
    a = (s.w.pos + 3 + 7) // 8
    s.stored(bytes(rng.randint(0, 256, size=200).astype(np.uint8)))
    s.fixed(); s.lits(rng.randint(0, 144, size=1021 - 2 - s.w.pos // 8)); s.end()     # (three header bits, eight a literal, seven the end-of-block)
    c = (s.w.pos + 3 + 7) // 8
    s.stored(bytes(rng.randint(0, 256, size=300).astype(np.uint8)), final=True)

    def claim(bl, a=a, c=c):
        assert (a, c) == (511, 1021) and [b.btype for b in bl] == [1, 0, 1, 0]
        assert (bl[1].bit_start + 3 + 7) // 8 == 511 and (bl[3].bit_start + 3 + 7) // 8 == 1021
    yield Case("stored: LEN across the chunk edge at byte 512, NLEN across the one at 1024", "valid", s.finish(), s.out, claim)

    s = W.Stream()
    s.stored(bytes(rng.randint(0, 256, size=507).astype(np.uint8)))
    s.dynamic(LL_WIN, D_FLAT, final=True)
    s.tokens([97, 98, (30, 400), 99, (258, 509)])

    def claim(bl):
        assert bl[0].btype == 0 and bl[0].bit_end == CHUNK_BITS == bl[1].bit_start and bl[1].btype == 2
    yield Case("stored: a block that ends on the chunk edge, a dynamic block behind it", "valid", done(s), s.out, claim)

    s = W.Stream()
    for k in range(20):
        s.stored(b"", pad=k & 1)
    s.fixed(final=True); s.lits(b"after twenty empty blocks")

    def claim(bl):
        assert [b.btype for b in bl] == [0] * 20 + [1] and not any(b.data for b in bl[:20])
    yield Case("stored: twenty empty blocks in a row", "valid", done(s), s.out, claim)

    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT); s.lits(rng.choice(ABCD, size=300)); s.end()
    s.stored(bytes(rng.randint(0, 256, size=700).astype(np.uint8)))
    s.dynamic(LL_WIN, D_FLAT, final=True)
    s.tokens([(30, 650), (258, 990), 97, (100, 1000 + 288)])

    def claim(bl):
        assert [b.btype for b in bl] == [2, 0, 2] and len(bl[0].data) == 300 and bl[2].matches()[1][1] > 700
    yield Case("stored: a block behind 300 literals, matches into both behind it", "valid", done(s), s.out, claim)


def sequence_cases():
    """tables, long_lim and lens[] from one block to the next: 15-bit codes, then short ones, then the fixed code, then one
    distance code -- and the other way round"""
    rng = np.random.RandomState(23)
    ll9 = W.random_complete_code(rng, 286, 200, must=(256, 97, 98, 257, 270, 285), max_len=9, deep=0.1)
    d9 = W.random_complete_code(rng, 30, 12, must=(0, 3, 10), max_len=9)

    def blk(s, kind, final):
        n = len(s.out)
        if kind == "15":
            s.dynamic(LL_PROBE, D_PROBE, final=final)
            s.tokens([65, 66, 0, 5, 11, 65, 65, (258, 1, 284), (240, 257, 284), 11, 66])
        elif kind == "9":
            s.dynamic(ll9, d9, final=final)
            s.tokens([97, 98, 97, (3, 1), 98, (24, 4), (258, 33), 97])
        elif kind == "fixed":
            s.fixed(final=final)
            s.tokens([1, 200, 255, (3, 2), 144, (100, 5), 0])
        else:
            s.dynamic(LL_WIN, [1], final=final)
            s.tokens([97, 100, (5, 1), 99, (33, 1), 98])
        s.end()

    for name, order in (("15-bit codes, codes of at most 9 bits, fixed, one distance code", ("15", "9", "fixed", "one")), ("the same the other way round", ("one", "fixed", "9", "15"))):
        s = W.Stream()
        for k, kind in enumerate(order + order):
            blk(s, kind, k == 7)

        def claim(bl, order=order):
            for b, kind in zip(bl, order + order):
                if kind == "15": assert b.btype == 2 and max(b.ll_lens) == 15 and max(b.d_lens) == 15 and 11 in b.tokens
                elif kind == "9": assert b.btype == 2 and max(b.ll_lens) <= 9 and max(b.d_lens) <= 9
                elif kind == "fixed": assert b.btype == 1
                else: assert b.btype == 2 and b.d_lens == [1]
        yield Case("block sequence: " + name, "valid", s.finish(), s.out, claim)


def largest_cases():
    for size in (65536, 65535):
        s = W.Stream()
        s.fixed(final=True)
        s.lits(np.random.RandomState(size & 0xff).randint(0, 256, size=300))
        while len(s.out) + 258 <= size:
            s.match(258, 300 - (len(s.out) % 7))
        if size - len(s.out) >= 3: s.match(size - len(s.out), 259)
        s.lits([7] * (size - len(s.out)))

        def claim(bl, size=size):
            assert sum(len(b.data) for b in bl) == size and len(bl[0].tokens) < 700
        yield Case("largest: ISIZE %d" % size, "valid", done(s), s.out, claim)
    # the largest payload a BGZF block holds: 65536 - 18 - 8 bytes
    s = W.Stream()
    s.fixed(); s.lits(b"the largest clen"); s.end()
    room = 65536 - 26 - ((s.w.pos + 3 + 7) // 8 + 4)
    s.stored(bytes(np.random.RandomState(77).randint(0, 256, size=room).astype(np.uint8)), final=True)
    payload = s.finish()

    def claim(bl, n=len(payload)):
        assert n == 65510
    yield Case("largest: a payload of 65510 bytes, the most a BGZF block holds", "valid", payload, s.out, claim)


def fuzz_seed():
    return int(os.environ.get("INFLATE_CRAFTED_SEED", 20261021))      # (soak runs: another seed per run)


def random_cases(count=200, seed=None):
    """random tokens over random complete codes with lengths 1 .. 15 in every alphabet, random block splits"""
    rng = np.random.RandomState(fuzz_seed() if seed is None else seed)
    for k in range(count):
        s = W.Stream()
        target = int(rng.choice([40, 700, 3000, 9000, 19000], p=[0.15, 0.25, 0.35, 0.15, 0.10]))
        n_blocks = int(rng.randint(1, 5))
        for bi in range(n_blocks):
            final = bi == n_blocks - 1
            goal = min(20000 - 300 * (n_blocks - bi), len(s.out) + target // n_blocks + 1)
            kind = rng.rand()
            if kind < 0.12:
                s.stored(bytes(rng.randint(0, 256, size=max(0, min(goal - len(s.out), int(rng.randint(0, 900))))).astype(np.uint8)), final=final)
                continue
            if kind < 0.3:
                s.fixed(final=final)
                lits, lsyms, dsyms = list(range(256)), list(range(257, 286)), list(range(30))
            else:
                n_lit, n_len, n_d = int(rng.choice([1, 2, 4, 30, 256])), int(rng.randint(0, 30)), int(rng.randint(1, 31))
                lits = [int(x) for x in rng.permutation(256)[:n_lit]]
                lsyms = [257 + int(x) for x in rng.permutation(29)[:n_len]]
                dsyms = sorted(int(x) for x in rng.permutation(30)[:n_d])
                if dsyms[0] > 3: dsyms[0] = int(rng.randint(0, 4))        # a distance the first bytes can reach
                ll = W.random_complete_code(rng, 286, 1 + n_lit + len(lsyms), must=[256] + lits + lsyms, deep=rng.rand())
                if len(dsyms) == 1 and rng.rand() < 0.5:
                    d = [0] * dsyms[0] + [1]
                else:
                    if len(dsyms) == 1: dsyms.append(dsyms[0] + 1)
                    d = W.random_complete_code(rng, 30, len(dsyms), must=dsyms, deep=rng.rand())
                hl = max(257, max([256] + lsyms) + 1)
                ll = ll[:int(rng.randint(hl, 287))]
                d = d[:int(rng.randint(max(dsyms) + 1, 31))]
                s.dynamic(ll, d, final=final, runs=rng.rand() < 0.8, hclen=None)
            p_match = rng.rand() * 0.7 if lsyms else 0.0
            while len(s.out) < goal:
                if len(s.out) and rng.rand() < p_match:
                    ds = [x for x in dsyms if R.DIST_BASE[x] <= len(s.out)]
                    if ds:
                        x = ds[rng.randint(len(ds))]
                        dist = min(len(s.out), R.DIST_BASE[x] + int(rng.randint(0, 1 << R.DIST_EXTRA[x])))
                        sym = lsyms[rng.randint(len(lsyms))]
                        s.match(R.LEN_BASE[sym - 257] + int(rng.randint(0, 1 << R.LEN_EXTRA[sym - 257])), dist, sym)
                        continue
                s.lit(lits[rng.randint(len(lits))])
            s.end()
        assert len(s.out) <= 20600
        yield Case("random stream %d" % k, "valid", s.finish(), s.out)


def table_cases():
    s = W.Stream()
    s.fixed(final=True)
    payload = done(s)

    def claim(bl):
        assert bl[0].btype == 1 and not bl[0].tokens
    yield Case("tables: an entry with ulen == 0 over an empty fixed block, handed in directly", "valid", payload, b"", claim, framed=False)
    s = W.Stream()
    s.fixed(final=True); s.lits(b"two more subfields"); s.match(50, 18)
    yield Case("tables: a frame with an extra subfield in front of BC and one behind it", "valid", done(s), s.out, lambda bl: None,
               before=W.subfield(b"AB", b"\x01\x02\x03"), after=W.subfield(b"BC", b"not the two-byte one") + W.subfield(b"ZZ", b""))


def invalid_cases():
    def fixed_with(write, name, why, note):
        s = W.Stream()
        s.fixed(final=True); s.lits(b"abcdefgh"); write(s); s.lits(b"z")
        return Case(name, "invalid", done(s), s.out, note=note, why=why)
    yield fixed_with(lambda s: s.symbol(286), "refused: symbol 286 in a fixed block", "length symbol 286", "sym > 285 behind the bit-by-bit decode")
    yield fixed_with(lambda s: s.symbol(287), "refused: symbol 287 in a fixed block", "length symbol 287", "sym > 285 behind the bit-by-bit decode")
    for d in (30, 31):
        yield fixed_with(lambda s, d=d: (s.symbol(260), s.symbol(d, True)), "refused: distance symbol %d in a fixed block" % d, "distance symbol %d" % d, "ds > 29 behind the bit-by-bit decode")

    s = W.Stream()
    s.fixed(); s.lits(b"ab"); s.end(); s.header(True, 3); s.raw(0x5a5a, 16)
    yield Case("refused: block type 3", "invalid", s.finish(), s.out, note="btype == 3u", why="reserved block type")
    s = W.Stream()
    s.stored(b"stored", final=True, nlen=6 ^ 0xfffe)
    yield Case("refused: NLEN is not ~LEN", "invalid", s.finish(), s.out, note="(len ^ nlen) != 0xffffu", why="NLEN")

    # an over-subscribed code in each alphabet
    cl = W.balanced_cl_lens(LL_WIN + D_FLAT)
    cl[0] = 1
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True, runs=False, cl_lens=cl, check=False); s.lits([97]); s.end()
    yield Case("refused: an over-subscribed code-length code", "invalid", s.finish(), s.out, note="build_tables of the code-length code", why="over-subscribed")
    ll = list(LL_WIN); ll[101] = 2
    s = W.Stream()
    s.dynamic(ll, D_FLAT, final=True, check=False); s.lits([97]); s.end()
    yield Case("refused: an over-subscribed literal/length code", "invalid", s.finish(), s.out, note="build_tables of the literal/length code", why="over-subscribed")
    d = list(D_FLAT); d[3] = 1
    s = W.Stream()
    s.dynamic(LL_WIN, d, final=True, check=False); s.lits([97]); s.end()
    yield Case("refused: an over-subscribed distance code", "invalid", s.finish(), s.out, note="build_tables of the distance code", why="over-subscribed")

    ops = W.rle_ops(LL_WIN + D_FLAT)
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True, ops=[(16, 3)] + ops, cl_lens=W.balanced_cl_lens([16] + [v if o == "len" else o for o, v in ops]), check=False); s.lits([97]); s.end()
    yield Case("refused: symbol 16 first", "invalid", s.finish(), s.out, note="sym == 16 with i == 0", why="repeat of the previous code length at the first")
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True, ops=ops[:-1] + [(17, 9)], cl_lens=W.balanced_cl_lens([17] + [v if o == "len" else o for o, v in ops]), check=False); s.lits([97]); s.end()
    yield Case("refused: a run past HLIT + HDIST", "invalid", s.finish(), s.out, note="i + rep > total", why="past HLIT + HDIST")
    ll = W.complete_code(257, {97: 1, 98: 1})
    s = W.Stream()
    s.dynamic(ll, [1], final=True, check=False); s.lits([97, 98, 98])
    yield Case("refused: no code for 256", "invalid", s.finish(), s.out, note="W.lens[256] == 0", why="no code for end-of-block")

    # dist == pos + 1: a long match (it ends its step), a short one inside a step, one with a distance code taken bit by bit
    for name, d_lens, toks, note in (("a long match", D_FLAT, [97, 98, 99, (40, 4)], "dist > pos at the step's last token"), ("a short match inside a step", D_FLAT, [97, 98, 99, (4, 4)], "D > mpos in the step"),
                                     ("a distance code taken bit by bit", W.complete_code(30, {3: 12, 0: 1}), [97, 98, 99, (4, 4)], "dist > pos behind the bit-by-bit decode")):
        s = W.Stream()
        s.dynamic(LL_WIN, d_lens, final=True)
        for t in toks:
            s.lit(t) if isinstance(t, int) else s.match(*t, check=False)
        s.lits([97, 98])
        yield Case("refused: dist == pos + 1, " + name, "invalid", done(s), s.out, note=note, why="beyond the 3 bytes")

    # the frame's ISIZE one under and one over what the tokens spell (the CRC32 is the right one)
    for name, toks, note in (("literals", [97] * 40, "n_lit > ulen - pos"), ("a short match", [97, 98, 99, (20, 2)], "total > ulen - pos"), ("a long match", [97, 98, (258, 1)], "pos + len > ulen")):
        s = W.Stream()
        s.dynamic(LL_WIN, D_FLAT, final=True); s.tokens(toks)
        yield Case("refused: one byte more than ISIZE, by " + name, "invalid", done(s), s.out, note=note, why="isize", isize=len(s.out) - 1)
    s = W.Stream()
    s.stored(b"one more than the table says", final=True)
    yield Case("refused: one byte more than ISIZE, by a stored block", "invalid", s.finish(), s.out, note="pos + len > ulen of a stored block", why="isize", isize=len(s.out) - 1)
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True); s.tokens([97, 98, 99, (20, 2), 100])
    payload = done(s)
    yield Case("refused: one byte less than ISIZE", "invalid", payload, s.out, note="pos != ulen behind the last block", why="isize", isize=len(s.out) + 1)
    yield Case("refused: a wrong CRC32", "invalid", payload, s.out, note="acc != B.crc", why="crc", crc=W.crc32_fast(s.out) ^ 0x8000)

    # no end-of-block: behind the payload come the trailer and zeros; the one-bit code of 'A' is zero, so literals follow until
    # ISIZE is passed -- and a fixed block, where the bits behind it must not spell the end-of-block (seven zeros)
    s = probe_stream(room=300)
    yield Case("refused: no end-of-block, 'A's to the end (dynamic)", "invalid", s.finish(), s.out, note="n_lit > ulen - pos (or pos + len > ulen)", why="the stream ends inside a block")
    for extra in range(64):
        s = W.Stream()
        s.fixed(final=True); s.lits(b"no end-of-block %d" % extra)
        s.w.align(1)
        if W.crc32_fast(s.out) & 0x7f:
            break
    yield Case("refused: no end-of-block (fixed)", "invalid", s.finish(), s.out, note="pos >= ulen / n_lit > ulen - pos at the token the trailer spells", why="the stream ends inside a block")
    # blocks that go on far behind clen: empty fixed blocks, ten bits each, nothing written; the table entry says 20 bytes
    s = W.Stream()
    for k in range(200):
        s.fixed(); s.end()
    yield Case("refused: blocks that go on 64 bytes and more behind clen (by a table entry)", "invalid", s.finish(), b"", note="bitpos > bit_end at a block's start", why="short", framed=False, clen=20)


def lenient_cases():
    ll = list(LL_WIN); ll[285] = 0
    s = W.Stream()
    s.dynamic(ll, D_FLAT, final=True, check=False); s.tokens([97, 98, 99, (20, 2), 100])
    yield Case("lenient: an incomplete literal/length code", "lenient", done(s), s.out, why="literal/length code: incomplete")
    d = list(D_FLAT); d[29] = 0
    s = W.Stream()
    s.dynamic(LL_WIN, d, final=True, check=False); s.tokens([97, 98, 99, (20, 2), 100])
    yield Case("lenient: an incomplete distance code of 29 symbols", "lenient", done(s), s.out, why="distance code: incomplete")
    ops = W.rle_ops(LL_WIN + D_FLAT)
    cl = W.balanced_cl_lens([v if o == "len" else o for o, v in ops] + [15])      # one more symbol than is used, then taken away
    cl[15] = 0
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True, ops=ops, cl_lens=cl, check=False); s.tokens([97, 98, 99, (20, 2), 100])
    yield Case("lenient: an incomplete code-length code", "lenient", done(s), s.out, why="code-length code: incomplete")
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True); s.tokens([97, 98, 99, (20, 2), 100]); s.end()
    assert s.w.n
    yield Case("lenient: ones in the padding behind the final block", "lenient", s.finish(1), s.out, why="non-zero padding")
    s = W.Stream()
    s.dynamic(LL_WIN, D_FLAT, final=True); s.tokens([97, 98, 99, (20, 2), 100]); s.end()
    yield Case("lenient: bytes behind the final block inside clen", "lenient", s.finish() + b"\x07trailing\xff", s.out, why="bytes after the final block")


@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for make in (long_code_cases, alphabet_cases, code_length_cases, ring_cases, lane_cases, window_cases, step_cases, stored_cases, sequence_cases,
                 largest_cases, random_cases, table_cases, invalid_cases, lenient_cases):
        out += list(make())
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def of_class(cls):
    return [c for c in all_cases() if c.cls == cls]

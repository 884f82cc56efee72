"""The yardsticks of tests/test_gpu_inflate_crafted.py, pinned without a GPU: the writer tests/deflate_write.py against zlib and
tests/deflate_ref.py, and every stream of tests/inflate_cases.py against both -- zlib gives the valid ones' bytes and refuses
the others as their class says, deflate_ref reads the valid ones back token by token, and each case is what its name says
(Case.claim over deflate_ref's Block objects: this code length on a token, this token at this bit, this distance at this
position in this step)."""
import functools
import re
import struct
import zlib

import numpy as np
import pytest

from tests import deflate_ref as R
from tests import deflate_write as W
from tests import inflate_cases as ic


@functools.lru_cache(maxsize=None)
def blocks_of(name):
    c = next(c for c in ic.all_cases() if c.name == name)
    return R.inflate_exact(c.payload)


def zlib_says(c):
    """"ok": the payload inflates, ends, and gives the frame's ISIZE and CRC32; else what is wrong"""
    try:
        out, eof, rest = ic.zlib_inflate(c.payload[:c.clen])
    except zlib.error as e:
        return "raises: %s" % e
    if not eof: return "short"
    if rest: return "bytes left over"
    if len(out) != c.isize: return "isize"
    if zlib.crc32(out) & 0xffffffff != c.crc: return "crc"
    return "ok" if out == c.want else "other bytes"


# ---- the writer -------------------------------------------------------------------------------------------------------------
def test_the_writer_round_trips_through_zlib_and_the_reader():
    rng = np.random.RandomState(4)
    assert W.crc32_fast(b"") == 0
    for n in (1, 2, 3, 100, 1000):
        data = bytes(rng.randint(0, 256, size=n).astype(np.uint8))
        assert W.crc32_fast(data) == zlib.crc32(data) & 0xffffffff
    assert W.crc32_fast(b"123456789") == R.crc32(b"123456789") == 0xCBF43926
    for n_used in (2, 3, 17, 100, 286):
        lens = W.random_complete_code(rng, 286, n_used, must=(256,))
        assert R.kraft(lens) == (W.FULL, n_used) and lens[256]
    lens = W.complete_code(286, {65: 1, 66: 2, 256: 15, 284: 15})
    assert (lens[65], lens[66], lens[256], lens[284]) == (1, 2, 15, 15) and R.kraft(lens)[0] == W.FULL
    assert sorted(set(W.complete_code(30, {}, spread=30))) == [4, 5]
    for lens in ([3, 3, 3, 0, 0, 0, 0, 7] + [0] * 140 + [5] * 9 + [0] * 12, [0] * 30, [8] * 2):
        for runs in (True, False):
            assert W.ops_lengths(W.rle_ops(lens, runs)) == lens
    # pad_to lands on the bit, whatever it is
    for bit in (600, 601, 777, 4096):
        s = W.Stream()
        s.dynamic(ic.LL_PROBE, ic.D_PROBE, final=True)
        s.pad_to(bit, {65: 1, 66: 2, 11: 14})
        s.lit(0)
        s.end()
        b = R.inflate_exact(s.finish())[0]
        assert b.token_bits[-1] == bit and zlib.decompressobj(-15).decompress(s.finish()) == bytes(s.out)
    # the frame: what deflate_ref's walker and the BGZF layout say
    s = W.Stream()
    s.fixed(final=True); s.lits(b"frame"); s.end()
    raw = W.bgzf_frame(s.finish(), s.out)
    (payload, crc, isize, bsize), = R.bgzf_payloads(raw)
    assert (payload, crc, isize, bsize) == (s.finish(), zlib.crc32(b"frame"), 5, len(raw)) and raw[:16] == b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0"
    raw = W.bgzf_frame(s.finish(), s.out, before=W.subfield(b"AB", b"xyz"), after=W.subfield(b"CD", b""))
    assert struct.unpack_from("<H", raw, 10)[0] == 7 + 6 + 4 and raw[12:19] == b"AB\x03\0xyz" and struct.unpack_from("<H", raw, 23)[0] == len(raw) - 1
    assert zlib.decompress(raw, 31) == b"frame"            # (zlib's gzip reader steps over the subfields)


# ---- the cases --------------------------------------------------------------------------------------------------------------
def test_the_table_has_what_the_tests_need():
    cases = ic.all_cases()
    assert len(ic.of_class("valid")) >= 250 and len(ic.of_class("invalid")) >= 20 and len(ic.of_class("lenient")) == 5
    assert sum(1 for c in cases if c.name.startswith("random stream")) == 200
    assert sum(len(c.want) for c in cases) < 2_500_000
    for c in cases:
        assert c.raw is None or len(c.raw) <= 65536, c.name
        if c.raw is not None and c.xlen == 6:
            assert R.bgzf_payloads(c.raw) == [(c.payload, c.crc, c.isize, len(c.raw))], c.name
        if c.cls == "invalid":
            assert c.note and c.why, c.name
        if c.cls == "valid" and not c.name.startswith("random stream"):
            assert c.claim is not None, c.name
    names = " ".join(c.name for c in cases)
    for off in range(49):
        assert "token %d bits in front" % off in names


@pytest.mark.parametrize("c", ic.of_class("valid"), ids=lambda c: c.name)
def test_valid_case(c):
    assert zlib_says(c) == "ok", c.name
    blocks = blocks_of(c.name)
    assert b"".join(b.data for b in blocks) == c.want and [b.bfinal for b in blocks] == [0] * (len(blocks) - 1) + [1]
    if c.claim:
        c.claim(blocks)


def test_the_largest_and_the_framed_cases_say_what_they_are():
    by = {c.name: c for c in ic.all_cases()}
    assert by["largest: ISIZE 65536"].isize == 65536 and struct.unpack("<I", by["largest: ISIZE 65536"].raw[-4:])[0] == 65536
    assert by["largest: ISIZE 65535"].isize == 65535
    c = by["largest: a payload of 65510 bytes, the most a BGZF block holds"]
    assert len(c.raw) == 65536 and len(c.payload) == 65510
    c = by["tables: a frame with an extra subfield in front of BC and one behind it"]
    assert c.xlen == 6 + 7 + 24 + 4 and zlib.decompress(c.raw, 31) == c.want and c.raw[12:14] == b"AB" and c.raw[19:21] == b"BC" and c.raw[25:27] == b"BC"
    assert [c.name for c in ic.all_cases() if c.raw is None] == ["stored: a block of 65535 bytes (no BGZF frame holds it: by a table entry)",
                                                                 "tables: an entry with ulen == 0 over an empty fixed block, handed in directly",
                                                                 "refused: blocks that go on 64 bytes and more behind clen (by a table entry)"]


def test_the_second_set_of_258_byte_distances_needs_the_remainder_fixed():
    """k_inflate takes i mod dist of an overlapping match by a float32 reciprocal and mends a quotient that came out one
    short.  At 1, 2, 3, 63, 64, 65, 257 it never does; the second case's distances are some of those where it does."""
    def one_short(dist):
        rcp = np.float32(1.0) / np.float32(dist)
        return [i for i in range(258) if i - int(np.float32(i) * rcp) * dist >= dist]
    assert not any(one_short(d) for d in (1, 2, 3, 31, 33, 63, 64, 65, 257))
    c = next(c for c in ic.all_cases() if c.name.startswith("steps: 258-byte matches at distances where the quotient"))
    dists = [t[1] for t in blocks_of(c.name)[0].matches()]
    assert dists == [41, 47, 55, 61, 83, 97, 141, 249] and all(one_short(d) for d in dists)


def test_random_streams_reach_every_code_length():
    """over the 200 random streams: literal/length and distance codes of every length 1 .. 15 on tokens, every block type"""
    ll, dd, types = set(), set(), set()
    for c in ic.all_cases():
        if c.name.startswith("random stream"):
            for b in blocks_of(c.name):
                types.add(b.btype)
                if b.btype == 2:
                    for t in b.tokens:
                        if isinstance(t, int): ll.add(b.ll_lens[t])
                        else:
                            ll.add(max(b.ll_lens[s] for s in range(257, b.hlit) if R.LEN_BASE[s - 257] <= t[0] < R.LEN_BASE[s - 257] + (1 << R.LEN_EXTRA[s - 257]) + (s == 284)))
                            dd.add(b.d_lens[W.distance_symbol(t[1])[0]])
    assert ll >= set(range(1, 16)) and dd >= set(range(1, 16)) and types == {0, 1, 2}


@pytest.mark.parametrize("c", ic.of_class("invalid"), ids=lambda c: c.name)
def test_invalid_case(c):
    verdict = zlib_says(c)
    assert verdict != "ok", c.name
    if c.why in ("isize", "crc", "short"):
        assert verdict == c.why
        if c.why != "short":
            assert b"".join(b.data for b in R.inflate_exact(c.payload)) == c.want
    else:
        with pytest.raises(R.DeflateError, match=re.escape(c.why)):
            R.inflate_exact(c.payload)


@pytest.mark.parametrize("c", ic.of_class("lenient"), ids=lambda c: c.name)
def test_lenient_case(c):
    """the strict reader refuses it for the one reason its name gives; zlib refuses it too, or (padding bits, bytes behind the
    stream: zlib's raw inflate does not look at either) gives exactly the bytes the tokens spell"""
    with pytest.raises(R.DeflateError, match=re.escape(c.why)):
        R.inflate_exact(c.payload)
    try:
        out, eof, rest = ic.zlib_inflate(c.payload)
    except zlib.error:
        assert "incomplete" in c.why
        return
    assert "incomplete" not in c.why and eof and out == c.want and (rest != b"") == ("bytes after" in c.why)
    assert zlib.crc32(c.want) & 0xffffffff == c.crc and len(c.want) == c.isize

"""The yardsticks of tests/test_gpu_codec.py, pinned without a GPU: the token-level reader tests/deflate_ref.py against zlib's own
streams and against hand-made streams it must refuse, the payloads of tests/deflate_cases.py against what their labels say, and
a Python model of the encoder's code-length routine on every histogram before the device sees it."""
import functools
import heapq
import zlib

import pytest

from tests import deflate_cases as dc
from tests import deflate_ref as R


# ---- deflate_ref against zlib ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_payloads():
    """a cut through every family, about 300 KB in all"""
    return tuple(_small_payloads())


def _small_payloads():
    for label, data, exp in dc.planted_distances():
        if label.endswith("plant 0") and (exp["group"][1] <= 4097 or exp["group"][1] == 32768):
            yield label, data, exp
    for label, data, exp in dc.planted_lengths():
        if label.endswith("plant 0") and exp["group"][2] == 0 and exp["group"][1] in dc.LENGTHS[::3] + [258, 259, 1000]:
            yield label, data, exp
    for label, data, exp in dc.matches_to_the_end():
        if label.endswith("plant 3") and len(data) < dc.PAYLOAD:
            yield label, data, exp
    for label, data, exp in dc.code_length_cases():
        if len(data) <= 8192:
            yield label, data, exp
    for label, data, exp in dc.size_cases():
        if len(data) <= 1793:
            yield label, data, exp
    yield from sorted(dc.fuzz_streams(), key=lambda c: len(c[1]))[:3]


def raw_deflate(data, level, strategy, flush_at=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(data[flush_at:]) + c.flush()


def check_blocks(blocks, data, what):
    assert b"".join(b.data for b in blocks) == data, what
    assert [b.bfinal for b in blocks] == [0] * (len(blocks) - 1) + [1], what
    pos = 0
    for b in blocks:
        for t in b.tokens:
            if isinstance(t, int):
                pos += 1
            else:
                length, dist, at = t
                assert 3 <= length <= 258 and 1 <= dist <= 32768 and at == pos and dist <= at, (what, t)
                pos += length
        if b.btype == 2:      # (deflate_ref raised already if a code were not complete: said again here, from the lengths)
            assert R.kraft(b.ll_lens)[0] == 32768 and R.kraft(b.cl_lens)[0] == 32768, what
            k, used = R.kraft(b.d_lens)
            assert k == 32768 or used == 0 or (used == 1 and k == 16384), what
            assert max(b.ll_lens + b.d_lens) <= 15 and max(b.cl_lens) <= 7, what
    assert pos == len(data), what


@pytest.mark.parametrize("strategy", [zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE])
@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_reader_expands_zlib_streams_to_their_input(level, strategy):
    types = set()
    for label, data, exp in small_payloads():
        for flush_at in (None, len(data) // 2):
            z = raw_deflate(data, level, strategy, flush_at)
            blocks = R.inflate_exact(z)
            check_blocks(blocks, data, (label, level, strategy, flush_at))
            types |= {b.btype for b in blocks}
            if flush_at is not None:    # the flush leaves an empty stored block on a byte boundary
                assert any(b.btype == 0 and not b.data and b.bit_end % 8 == 0 for b in blocks[:-1]), label
    assert types >= ({0} if level == 0 else {0, 1} if strategy == zlib.Z_FIXED else {0, 2})


def test_reader_sees_the_planted_tokens_in_zlib_streams():
    """zlib -9 (a chained hash table: nothing is lost within its window of 32768 - 262) finds every plant, and the reader
    shows it where the case says it is: the expectations can be met, and shows() reads them right."""
    seen = 0
    for label, data, exp in small_payloads():
        if not ({"dist", "token_at", "end_match", "one_match", "no_match"} & set(exp)) or exp.get("dist", 0) > 32768 - 262:
            continue
        tokens = [t for b in R.inflate_exact(raw_deflate(data, 9, zlib.Z_DEFAULT_STRATEGY)) for t in b.tokens]
        if exp.get("no_match"):      # (zlib matches from 3 bytes and inside a step: a run is matched)
            continue
        assert dc.shows(exp, tokens, len(data)) == [], label
        assert dc.wrong_tokens(exp, tokens) == [], label
        seen += 1
    assert seen > 40
    # and shows() says what is missing when it is
    assert dc.shows({"dist": 300, "copy": (300, 10)}, [1, 2, (5, 299, 300)], 9)
    assert dc.shows({"token_at": (10, 258, 4096)}, [(257, 4096, 10)], 9) and dc.wrong_tokens({"token_at": (10, 258, 4096)}, [(257, 4096, 10)])
    assert dc.shows({"end_match": 20}, [(5, 3, 14), 7], 20) and dc.shows({"end_match": 20}, [(5, 3, 14)], 20)
    assert dc.shows({"end_match": 20}, [7, (5, 3, 15)], 20) == []
    assert dc.groups_missing([({"group": 1}, ["x"]), ({"group": 1}, []), ({"group": 2}, ["y"]), ({}, ["z"]), ({}, [])]).keys() == {2, ("alone", 3)}


# ---- streams the reader must refuse -----------------------------------------------------------------------------------------
class BitsOut:
    def __init__(self):
        self.v, self.n = 0, 0

    def bits(self, value, n):        # least significant bit first
        self.v |= value << self.n
        self.n += n

    def code(self, code, n):         # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.bits((code >> k) & 1, 1)

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def dynamic_header(w, ll_lens, d_lens, bfinal=1):
    """every code length as a 4-bit symbol of a flat code-length code (symbols 0 .. 15)"""
    w.bits(bfinal, 1); w.bits(2, 2); w.bits(len(ll_lens) - 257, 5); w.bits(len(d_lens) - 1, 5); w.bits(15, 4)
    for s in R.CL_ORDER:
        w.bits(4 if s < 16 else 0, 3)
    for l in list(ll_lens) + list(d_lens):
        w.code(l, 4)


def codes_of(lens):
    return {sym: (key ^ (1 << lens[sym]), lens[sym]) for key, sym in R.canonical(lens).items()}


def test_reader_refuses_what_the_rfc_forbids():
    def ll(**by_symbol):
        lens = [0] * 286
        for s, l in by_symbol.items():
            lens[int(s[1:])] = l
        return lens

    # a well-formed block of this make is read: 'a', 'b', a match (3, 2), end-of-block
    good = ll(s97=2, s98=2, s256=2, s257=2)
    w = BitsOut(); dynamic_header(w, good, [1] + [0] * 29)
    c = codes_of(good)
    for s in (97, 98, 257):
        w.code(*c[s])
        if s == 257:
            w.code(0, 1)             # distance symbol 0, the one-bit code: distance 1
    w.code(*c[256])
    (b,), used = R.inflate(w.bytes())
    assert b.data == b"abbbb" and b.tokens == [97, 98, (3, 1, 2)] and b.hlit == 286 and b.hdist == 30 and used == len(w.bytes())
    assert b.d_lens == [1] + [0] * 29 and b.cl_lens == [4] * 16 + [0, 0, 0]

    def refused(w, word):
        with pytest.raises(R.DeflateError) as e:
            R.inflate_exact(w.bytes())
        assert word in str(e.value), str(e.value)

    w = BitsOut(); dynamic_header(w, ll(s97=1, s98=1, s256=1), [0] * 30); refused(w, "over-subscribed")
    w = BitsOut(); dynamic_header(w, ll(s97=2, s256=2), [0] * 30); refused(w, "incomplete")
    w = BitsOut(); dynamic_header(w, ll(s97=1, s256=1), [2, 2] + [0] * 28); refused(w, "incomplete")      # two 2-bit distance codes
    w = BitsOut(); dynamic_header(w, ll(s97=1, s256=1), [2] + [0] * 29); refused(w, "incomplete")         # one, but not of one bit
    w = BitsOut(); dynamic_header(w, ll(s97=1, s98=1), [0] * 30); refused(w, "end-of-block")              # no code for 256
    # fixed code: a match before any output; a literal and then nothing; a literal, end-of-block and a stray bit in the padding
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(1, 7); w.code(0, 5); w.code(0, 7); refused(w, "beyond the 0 bytes")
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(0x30 + 65, 8); refused(w, "ends inside a block")
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(0x30 + 65, 8); w.code(0, 7); w.bits(0, 1); w.bits(1, 1); refused(w, "padding")
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(0x30 + 65, 8); w.code(0, 7); w.bits(0, 13); refused(w, "after the final block")
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(0x30 + 65, 8); w.code(0, 7)
    assert R.inflate_exact(w.bytes())[0].data == b"A"
    # a match in a block that declares no distance code, a distance symbol 30, block type 3
    w = BitsOut(); dynamic_header(w, good, [0] * 30); w.code(*c[97]); w.code(*c[257]); w.code(0, 1); refused(w, "without a distance code")
    w = BitsOut(); w.bits(1, 1); w.bits(1, 2); w.code(0x30 + 65, 8); w.code(1, 7); w.code(30, 5); refused(w, "distance symbol 30")
    w = BitsOut(); w.bits(1, 1); w.bits(3, 2); refused(w, "reserved")
    # zlib refuses the same over-subscribed, incomplete and too-far streams
    for lens, d in ((ll(s97=1, s98=1, s256=1), [0] * 30), (ll(s97=2, s256=2), [0] * 30)):
        w = BitsOut(); dynamic_header(w, lens, d)
        with pytest.raises(zlib.error):
            zlib.decompressobj(-15).decompress(w.bytes() + bytes(8))
    assert R.crc32(b"123456789") == 0xcbf43926 == zlib.crc32(b"123456789")


# ---- the cases mean what they say -------------------------------------------------------------------------------------------
def huffman_depth(freq):
    heap = [(f, 0) for f in freq if f]
    heapq.heapify(heap)
    while len(heap) > 1:
        (f1, d1), (f2, d2) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (f1 + f2, max(d1, d2) + 1))
    return heap[0][1]


def with_end_of_block(hist):
    return list(hist) + [1] + [0] * 29


def shannon(freq):
    total = sum(freq)
    return [0 if not f else next(l for l in range(1, 64) if (f << l) >= total) for f in freq]


def test_planted_copies_are_exactly_as_long_as_they_say():
    n = 0
    for label, data, exp in dc.planted_lengths():
        p, length = exp["copy"]
        s = p - 4096
        assert p % 128 == exp["group"][2] and exp["token_at"] == (p, min(length, 258), 4096)
        assert data[p:p + length] == data[s:s + length] and data[p + length] != data[s + length] and data[p - 1] != data[s - 1], label
        assert data.count(data[s:s + 4]) == 2 or length < 6, label       # (the match at p has one candidate)
        assert dc.slot_kept(data, s, p), label
        n += 1
    assert n == len(dc.LENGTHS) * len(dc.OFFSETS) * dc.N_SEEDS
    assert set(dc.LENGTHS) >= {b for b in R.LEN_BASE if b >= 4} | {257, 259, 300, 516, 1000} and min(dc.LENGTHS) == 4      # every length code's first length
    for label, data, exp in dc.planted_distances():
        d, rlen = exp["copy"]
        assert data[d:d + rlen] == data[:rlen] and len(data) == d + rlen and len(set(data[rlen:d])) == 1 and data[rlen] not in data[:rlen], label
        assert ("dist" in exp) == (128 <= d <= 32768)
    wanted = {128, 129, 32767, 32768, 32769} | {b for b in R.DIST_BASE if b > 128}
    assert wanted <= set(dc.DIST_EDGES) and {b - 1 for b in R.DIST_BASE if b > 129} <= set(dc.DIST_EDGES)
    sizes = set()
    for label, data, exp in dc.matches_to_the_end():
        at, k = exp["copy"]
        n_bytes = len(data)
        assert 5 <= k <= 40 and at + k == n_bytes and data.count(data[at:]) == 2 and 0 < at - data.find(data[at:]) <= 30000, label
        assert data[at - 1] != data[data.find(data[at:]) - 1], label
        assert ("end_match" in exp) == (n_bytes >= 132)
        sizes.add(n_bytes)
    assert sizes == {130, 131, 132, 133, 1000, 1001, 1002, 1003, 57344}
    assert {len(d) for _, d, _ in dc.size_cases()} == set(dc.SIZES) and len(dc.SIZES) == 33
    blocks = dc.unlike_blocks()
    assert len(blocks) == 63 * dc.PAYLOAD + 1
    alike = dc.repeated_preamble_blocks(16)
    assert len(alike) == 15 * dc.PAYLOAD + 1
    for k in range(15):
        blk = alike[k * dc.PAYLOAD:(k + 1) * dc.PAYLOAD]
        assert blk[:60] == blk[60:120] == alike[:60] and len(set(blk[120:])) == 1 and blk[120] not in blk[:120], k
    assert len({alike[k * dc.PAYLOAD + 120] for k in range(15)}) == 15
    assert not dc.slot_kept(b"abcd" + bytes(200) + b"abcdxabcd", 4 + 200, 4 + 200 + 5 + 128) and dc.slot_kept(b"abcd" + bytes(300), 0, 256)
    streams = list(dc.fuzz_streams())
    assert len(streams) == 60 and min(len(d) for _, d, _ in streams) < 300 and max(len(d) for _, d, _ in streams) > 300_000
    assert [d for _, d, _ in dc.fuzz_streams()] == [d for _, d, _ in streams]       # seeded


def test_code_length_histograms_are_what_their_labels_say():
    cases = {label: (data, exp) for label, data, exp in dc.code_length_cases()}
    for label, (data, exp) in cases.items():
        assert [data.count(bytes([v])) for v in range(256)] == exp["hist"], label
    fib = with_end_of_block(cases["Fibonacci ladder (Huffman depth above 15)"][1]["hist"])
    assert huffman_depth(fib) > 15
    below = with_end_of_block(cases["255 bytes just below 1/256 and one above (the maximal slack)"][1]["hist"])
    assert sorted(shannon(below)[:256]).count(9) == 255 and sum(below) == dc.PAYLOAD + 1
    pow2 = with_end_of_block(cases["exact powers of two"][1]["hist"])
    assert sum(1 << (15 - min(l, 15)) for l in shannon(pow2) if l) == 32768
    over = with_end_of_block(cases["three times powers of two and two rare bytes (Kraft above one at 15 bits)"][1]["hist"])
    assert sum(1 << (15 - min(l, 15)) for l in shannon(over) if l) > 32768
    assert sorted(set(cases["uniform over 256 (the largest literal-only block)"][1]["hist"])) == [224]


# ---- the encoder's code lengths, modelled -----------------------------------------------------------------------------------
def build_lengths_model(freq, max_sweeps=64):
    """A transcription of build_lengths() of bramble_amd/csrc/codec_kernels.hip, the wave's lanes unrolled into index order.
    Returns (lengths, lengthening steps, sweeps of the slack loop); raises if the slack loop has not ended after max_sweeps."""
    n, total, used = len(freq), sum(freq), sum(1 for f in freq if f)
    if used == 0:
        return [0] * n, 0, 0
    if used == 1:
        return [1 if f else 0 for f in freq], 0, 0
    lens, k15 = [0] * n, 0
    for i, f in enumerate(freq):
        if f:
            ll = 1
            while ll < 15 and (f << ll) < total:
                ll += 1
            lens[i] = ll
            k15 += 1 << (15 - ll)
    longer = 0
    while k15 > 32768:
        live = [(freq[i], i) for i in range(n) if lens[i] and lens[i] < 15]
        if not live:
            break
        _, pick = min(live)
        k15 -= 1 << (15 - lens[pick] - 1)
        lens[pick] += 1
        longer += 1
    slack, sweeps = 32768 - k15, 0
    while slack > 0:
        sweeps += 1
        if sweeps > max_sweeps:
            raise RuntimeError("the slack loop made %d sweeps and %d units are left" % (max_sweeps, slack))
        for l in range(2, 16):
            if slack <= 0:
                break
            step = 1 << (15 - l)
            if step > slack:
                continue
            can, taken = slack // step, 0
            for i in range(n):
                if taken >= can:
                    break
                if lens[i] == l:
                    lens[i] = l - 1
                    taken += 1
            slack -= taken * step
    return lens, longer, sweeps


# A sweep that ends with slack left has shortened EVERY symbol of the lengths whose step fits that slack (had one stayed, less
# than its step would be left), and the slack is a multiple of the longest code's step, so the longest code gets one bit shorter
# per sweep: 15 bits come down to 1 in 14 sweeps, and one more sweep hands out what is left.
MAX_SWEEPS = 15


def checked_code_length_cases():
    """The code-length cases whose histograms the model turns into a complete code of at most 15 bits within MAX_SWEEPS sweeps,
    as a list: what tests/test_gpu_codec.py sends to the device.  A histogram that fails here has not been near a GPU (a slack
    loop that does not end would hang a wave)."""
    out, worst = [], (0, 0, "")
    for label, data, exp in dc.code_length_cases():
        lens, longer, sweeps = build_lengths_model(with_end_of_block(exp["hist"]), max_sweeps=MAX_SWEEPS)
        assert R.kraft(lens)[0] == 32768 and max(lens) <= 15, (label, R.kraft(lens))
        assert all((l > 0) == (f > 0) for l, f in zip(lens, with_end_of_block(exp["hist"]))), label
        worst = max(worst, (sweeps, longer, label))
        out.append((label, data, dict(exp, model_sweeps=sweeps, model_longer=longer)))
    return out, worst


def test_code_length_model_ends_with_a_complete_code_on_every_case():
    cases, worst = checked_code_length_cases()
    assert len(cases) >= 20
    print("build_lengths model: at most %d sweeps of the slack loop (%d lengthening steps) on %r" % worst)
    by = {label: exp for label, _, exp in cases}
    assert by["three times powers of two and two rare bytes (Kraft above one at 15 bits)"]["model_longer"] >= 1    # the middle phase is reached
    assert by["exact powers of two"]["model_sweeps"] == 0 and by["exact powers of two"]["model_longer"] == 0
    assert by["255 bytes just below 1/256 and one above (the maximal slack)"]["model_sweeps"] >= 1
    # the distance alphabet, and histograms with matches in them: every token histogram zlib -1 and -9 make of the cases
    for label, data, exp in dc.code_length_cases():
        for level in (1, 9):
            fl, fd = [0] * 286, [0] * 30
            fl[256] = 1
            for b in R.inflate_exact(raw_deflate(data[:20000], level, zlib.Z_DEFAULT_STRATEGY)):
                for t in b.tokens:
                    if isinstance(t, int):
                        fl[t] += 1
                    else:
                        fl[257 + max(k for k in range(29) if R.LEN_BASE[k] <= t[0])] += 1
                        fd[max(k for k in range(30) if R.DIST_BASE[k] <= t[1])] += 1
            for freq in (fl, fd):
                lens, longer, sweeps = build_lengths_model(freq, max_sweeps=MAX_SWEEPS)
                used = sum(1 for f in freq if f)
                assert used <= 1 or R.kraft(lens)[0] == 32768, (label, level)
                assert max(lens) <= 15

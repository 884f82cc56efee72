"""BGZF deflate on the device (k_deflate_dynamic / k_deflate_fixed / k_bgzf_compact).  Any inflater must reproduce the input and
the block framing must be valid BGZF (header, BSIZE, CRC32, ISIZE): zlib, gzip and the device's own k_inflate read every output
back.  Beyond that the blocks are read token by token with tests/deflate_ref.py, a DEFLATE reader written from RFC 1951: block
type, code lengths, and the matches the payloads of tests/deflate_cases.py plant at the edges of the format (distance 32768,
length 258, every code boundary) and of the parse (lanes 0 and 63 of a half-round, the payload's last byte).  The compressed
bytes themselves are compared with no other encoder's: they are not part of the parity contract."""
import gzip
import io
import struct
import zlib

import numpy as np
import pytest

from bramble_amd import lib, synth
from tests import deflate_cases as dc
from tests import deflate_ref as R
from tests.test_deflate_cases_cpu import build_lengths_model, checked_code_length_cases

pytestmark = pytest.mark.gpu


def _ctx():
    idx = lib.Index({"refnames": ["chr1"], "transcripts": [{"id": "t", "ref_id": 0, "strand": "+", "exons": [[10, 50]]}]}, device=0)
    return idx, lib.Context(idx)


def inflate_blocks(raw):
    """Walk BGZF blocks, inflate each payload with zlib, verify CRC32 / ISIZE; returns (data, n_blocks, max_block)."""
    raw = bytes(raw)
    p, out, nb, mx = 0, [], 0, 0
    while p < len(raw):
        assert raw[p:p + 4] == b"\x1f\x8b\x08\x04" and raw[p + 12:p + 16] == b"BC\x02\x00"
        bsize = struct.unpack_from("<H", raw, p + 16)[0] + 1
        payload = raw[p + 18:p + bsize - 8]
        crc, isize = struct.unpack_from("<II", raw, p + bsize - 8)
        d = zlib.decompressobj(-15)
        data = d.decompress(payload)
        assert d.eof and d.unused_data == b""
        assert len(data) == isize and (zlib.crc32(data) & 0xffffffff) == crc
        out.append(data)
        nb += 1
        mx = max(mx, bsize)
        p += bsize
    return b"".join(out), nb, mx


def payloads():
    rng = np.random.RandomState(9)
    text = (b"@read%07d\tACGTACGTTTGACCA\t+\tIIIIHHHGGFF###\n" * 40000)
    yield "one byte", np.frombuffer(b"\x7f", dtype=np.uint8)
    yield "one symbol only", np.full(5000, 65, dtype=np.uint8)
    yield "two symbols", np.frombuffer(b"ab" * 3 + b"a" * 50 + b"b", dtype=np.uint8)
    yield "skewed (long codes for rare bytes)", np.concatenate([np.full(56000, 7, dtype=np.uint8), np.arange(256, dtype=np.uint8)])
    yield "three bytes", np.frombuffer(b"abc", dtype=np.uint8)
    yield "zeros", np.zeros(200_000, dtype=np.uint8)
    yield "random (incompressible, bytes >= 144 take 9 bits)", rng.randint(0, 256, size=300_001).astype(np.uint8)
    yield "high bytes", rng.randint(144, 256, size=57344 * 2).astype(np.uint8)
    yield "text", np.frombuffer(text, dtype=np.uint8)
    yield "block - 1", rng.randint(65, 70, size=57343).astype(np.uint8)
    yield "block", rng.randint(65, 70, size=57344).astype(np.uint8)
    yield "block + 1", rng.randint(65, 70, size=57345).astype(np.uint8)
    yield "long runs and far repeats", np.concatenate([np.tile(rng.randint(0, 256, size=40000).astype(np.uint8), 5),
                                                       np.repeat(rng.randint(0, 256, size=300).astype(np.uint8), 700)])


@pytest.mark.parametrize("dynamic", [1, 0])
def test_device_deflate_round_trips(dynamic):
    """dynamic = 1: k_deflate_dynamic (per-block Huffman codes, the default); 0: k_deflate_fixed."""
    import torch
    idx, ctx = _ctx()
    ctx.set_param("deflate_dynamic", dynamic)
    for label, data in payloads():
        src = torch.from_numpy(data.copy()).to("cuda:0")
        z = ctx.bgzf_deflate_device(src, 0).cpu().numpy().tobytes()
        got, nb, mx = inflate_blocks(z)
        assert got == data.tobytes(), label
        assert nb == (len(data) + 57343) // 57344 and mx <= 65536, label
        assert gzip.GzipFile(fileobj=io.BytesIO(z)).read() == data.tobytes(), label   # a second, independent reader
    ctx.close()
    idx.close()


def test_device_deflate_compresses_projected_stream():
    ann = synth.Annotation("G", n_genes=1500, n_refs=3)
    b = ann.reads(8000, "pe", with_records=1)
    stream, roff, rlen = synth.Annotation.frame_records(b)
    idx = lib.Index(ann.as_dict(), device=0)
    ctx = lib.Context(idx)
    cfg = lib.make_config()
    plain, c1 = ctx.project_bam_bundle(cfg, stream, roff, rlen, np.arange(3, dtype=np.int32))
    packed, c2 = ctx.project_bam_bundle(cfg, stream, roff, rlen, np.arange(3, dtype=np.int32), bgzf_on_device=True)
    assert c1 == c2
    got, nb, mx = inflate_blocks(packed.tobytes())
    assert got == plain.tobytes()
    assert len(packed) < 0.5 * len(plain)       # the stream repeats every read once per transcript
    ctx.close()
    idx.close()


# ---- token by token -------------------------------------------------------------------------------------------------------
SLOT = 65536                 # DEFLATE_SLOT of kernels.h, and the largest block BSIZE can state
BOUND = {1: 64876, 0: 64540}  # the largest block either coder can make of 57344 bytes, as argued at DEFLATE_PAYLOAD in kernels.h
LARGEST = {1: 0, 0: 0}       # the largest BGZF block of this run, per mode


@pytest.fixture(scope="module")
def codec():
    idx, ctx = _ctx()
    yield ctx
    ctx.close()
    idx.close()
    for dynamic in (1, 0):
        if LARGEST[dynamic]:
            print("\nlargest BGZF block of this run, deflate_dynamic = %d: %d bytes; bound %d, slot %d" % (dynamic, LARGEST[dynamic], BOUND[dynamic], SLOT))


def deflate_checked(ctx, data, dynamic, what):
    """data -> the device's BGZF bytes, after zlib (CRC32, ISIZE, BSIZE, block count, block size), gzip and the device's own
    inflater have each reproduced the input and every block has stated the mode's block type"""
    import torch
    ctx.set_param("deflate_dynamic", dynamic)
    z = ctx.bgzf_deflate_device(torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to("cuda:0"), 0).cpu().numpy().copy()
    raw = z.tobytes()
    got, nb, mx = inflate_blocks(raw)
    assert got == data, what
    assert nb == (len(data) + 57343) // 57344 and mx <= BOUND[dynamic] <= SLOT, (what, nb, mx)
    LARGEST[dynamic] = max(LARGEST[dynamic], mx)
    assert gzip.GzipFile(fileobj=io.BytesIO(raw)).read() == data, what
    for payload, crc, isize, bsize in R.bgzf_payloads(raw):
        assert payload[0] & 7 == (5 if dynamic else 3), what          # BFINAL, then BTYPE 2 (dynamic) or 1 (fixed)
    blocks, consumed, total = lib.bgzf_scan(z)
    assert consumed == z.size and total == len(data) and len(blocks) == nb, what
    back = ctx.bgzf_inflate_device(torch.from_numpy(z).to("cuda:0"), blocks)
    assert back.cpu().numpy().tobytes() == data, what
    return raw


def tokens_checked(raw, dynamic, what):
    """[(Block, first input byte)] of the device's BGZF bytes: one DEFLATE block per BGZF block, final, of the mode's type,
    every match 4 .. 258 long and 1 .. 32768 back; token positions count from the block's first byte"""
    out = []
    for k, blocks in enumerate(R.walk_bgzf(raw)):
        assert len(blocks) == 1 and blocks[0].bfinal == 1 and blocks[0].btype == (2 if dynamic else 1), what
        for length, dist, pos in blocks[0].matches():
            assert 4 <= length <= 258 and 1 <= dist <= 32768 and dist <= pos, (what, length, dist, pos)
        out.append(blocks[0])
    return out


def check_plants(ctx, dynamic, cases, pad, every=False):
    """pad: every payload is filled up to a whole block with a run of its last byte and all go through the encoder in one
    call, one plant per block (nothing about a plant's end is expected then); otherwise one call each.  every: each plant
    must show what it expects, not one of its group"""
    cases = list(cases)
    if pad:
        assert all(len(d) <= dc.PAYLOAD and "end_match" not in e for _, d, e in cases)
        raw = deflate_checked(ctx, b"".join(d + d[-1:] * (dc.PAYLOAD - len(d)) for _, d, _ in cases), dynamic, cases[0][0])
        per_case = tokens_checked(raw, dynamic, cases[0][0])
    else:
        per_case = []
        for label, data, exp in cases:
            blocks = tokens_checked(deflate_checked(ctx, data, dynamic, label), dynamic, label)
            assert len(blocks) == 1
            per_case.append(blocks[0])
    results = []
    for (label, data, exp), block in zip(cases, per_case):
        assert block.data[:len(data)] == data, label
        tokens = [t for t in block.tokens if isinstance(t, int) or t[2] < len(data)] if pad else block.tokens
        assert dc.wrong_tokens(exp, tokens) == [], (label, dc.wrong_tokens(exp, tokens))
        results.append((exp, dc.shows(exp, tokens, len(data))))
    found = {}
    for exp, missing in results:
        found.setdefault(exp["group"], []).append(not missing)
    print("plants that show what their group expects, of %d each: fewest %d, in all %d of %d"
          % (dc.N_SEEDS, min(sum(v) for v in found.values()), sum(sum(v) for v in found.values()), len(results)))
    assert dc.groups_missing(results) == {}
    if every:
        assert [missing for exp, missing in results if missing] == []


@pytest.mark.parametrize("dynamic", [1, 0])
def test_matches_at_every_distance_code_boundary(codec, dynamic):
    """128, 129, every distance code's first distance and the one before it, 32767, 32768: of eight seeds planted twice that far
    apart at least one is matched at exactly that distance.  At 32769 and below 128 only the round trip is asked for."""
    check_plants(codec, dynamic, dc.planted_distances(), pad=True)


@pytest.mark.parametrize("offset", dc.OFFSETS)
@pytest.mark.parametrize("dynamic", [1, 0])
def test_matches_of_every_length_code_boundary(codec, dynamic, offset):
    """A copy of exactly L bytes 4096 back, L at every length code's first length, 257, 258 and beyond (split: 258 first),
    starting in lane 0, 1, 62 or 63 of either half-round: a token of exactly min(L, 258) at that position in every plant (the
    plants are those whose table slot nothing overwrites, tests/deflate_cases.py::slot_kept)."""
    check_plants(codec, dynamic, dc.planted_lengths([offset]), pad=True, every=True)


@pytest.mark.parametrize("dynamic", [1, 0])
def test_matches_that_end_on_the_last_byte(codec, dynamic):
    """130 .. 133, 1000 .. 1003 and a whole block of bytes whose last 5 to 40 copy an earlier stretch: the last token is a match
    that ends on the last byte (every n mod 4: the byte-wise tail of the length comparison), in every plant -- the stretch is
    among the payload's few distinct bytes, nothing overwrites its table entries.  130 and 131 bytes are only round-tripped
    (tests/deflate_cases.py says why)."""
    check_plants(codec, dynamic, dc.matches_to_the_end(), pad=False, every=True)


@pytest.mark.parametrize("dynamic", [1, 0])
def test_code_lengths(codec, dynamic):
    """Dynamic blocks: both codes as the header states them are complete (the distance code may be empty or the single one-bit
    code), at most 15 bits, HLIT 286, HDIST 30, the flat 4-bit code-length code -- and they are the lengths the model of
    build_lengths (tests/test_deflate_cases_cpu.py, which has ended on these histograms before they come here) makes of the
    block's own token histogram.  The lengthening phase (Kraft sum above one once codes are held at 15 bits) is NOT reached
    on the device by these payloads: it needs token counts of almost exactly T / 2^k beside rare symbols, and the matcher turns
    the runs of the heavy bytes of such a byte histogram into matches.  The blocks that do reach it are printed (none so far);
    that phase is checked in the model only."""
    cases, _ = checked_code_length_cases()
    largest, lengthened = (0, ""), []
    for label, data, exp in cases:
        raw = deflate_checked(codec, data, dynamic, label)
        largest = max(largest, (len(raw), label))
        (b,) = tokens_checked(raw, dynamic, label)
        assert dc.shows(exp, b.tokens, len(data)) == [], label
        if not dynamic:
            continue
        assert (b.hlit, b.hdist, b.hclen) == (286, 30, 19) and b.cl_lens == [4] * 16 + [0, 0, 0], label
        assert R.kraft(b.ll_lens)[0] == 32768 and max(b.ll_lens + b.d_lens) <= 15, label
        k, used = R.kraft(b.d_lens)
        assert k == 32768 or used == 0 or (used == 1 and k == 16384), (label, b.d_lens)
        if exp.get("no_match"):
            assert b.d_lens == [0] * 30, label
        if exp.get("one_match"):
            assert sorted(b.d_lens) == [0] * 29 + [1], label
        fl, fd = [0] * 286, [0] * 30
        fl[256] = 1
        for t in b.tokens:
            if isinstance(t, int):
                fl[t] += 1
            else:
                fl[257 + max(s for s in range(29) if R.LEN_BASE[s] <= t[0])] += 1
                fd[max(s for s in range(30) if R.DIST_BASE[s] <= t[1])] += 1
        (ll_model, ll_longer, _), (d_model, d_longer, _) = build_lengths_model(fl), build_lengths_model(fd)
        assert b.ll_lens == ll_model and b.d_lens == d_model, label
        if ll_longer or d_longer:
            lengthened.append((label, ll_longer, d_longer))
    print("largest block of the code-length cases, deflate_dynamic = %d: %d bytes (%s); bound %d, slot %d" % (dynamic, largest[0], largest[1], BOUND[dynamic], SLOT))
    assert largest[0] <= BOUND[dynamic] <= SLOT
    if dynamic:
        print("blocks whose token histogram takes build_lengths through its lengthening phase (Kraft sum above one at 15 bits): %r" % (lengthened,))


@pytest.mark.parametrize("dynamic", [1, 0])
def test_sizes_next_to_the_parse_step_the_crc_chunk_and_the_block(codec, dynamic):
    """1 .. 9, 63 .. 65, 127 .. 132, the CRC fold's 896-byte lane chunks (895 .. 897, 1791 .. 1793, a block + 895 .. 897) and
    one and two blocks, +- 1: random bytes and a short period, one call each."""
    for label, data, exp in dc.size_cases():
        raw = deflate_checked(codec, data, dynamic, label)
        if len(data) <= 1793 or "period" in label or len(data) == dc.PAYLOAD + 1:
            tokens_checked(raw, dynamic, label)


def test_one_wave_takes_many_blocks(codec):
    """deflate_waves = 4: four persistent waves share 64 blocks, each unlike the one before (random, zeros, text, two letters,
    far repeats; the last is one byte), so what a wave keeps from one block to the next -- bit buffer, histograms, the code
    tables written over them, token list -- shows.  The bytes must be those of the default sizing, where nearly every block has
    a fresh wave: a block's bytes depend on neither the wave nor its past.
    The hash table needs a second input.  A step looks its 128 positions up before it inserts them, and a candidate need only
    lie at most 32768 below or AT the position and hold the same four bytes; in whole blocks of unlike bytes a table left from
    the last block holds positions near that block's end, which are above the position or overwritten by then.  So 15 blocks
    that begin with the same 60 bytes twice within the first step and go on with one repeated byte: a table left uncleared
    hands the second 60 their own positions (distance 0), a cleared one has nothing for them."""
    data = dc.unlike_blocks(64)
    assert len(data) < 3_700_000
    head = data[:9 * dc.PAYLOAD + 1]
    want, want_head = deflate_checked(codec, data, 1, "default sizing"), deflate_checked(codec, head, 1, "default sizing, ten blocks")
    codec.set_param("deflate_waves", 4)
    try:
        got = deflate_checked(codec, data, 1, "deflate_waves = 4")
        codec.set_param("deflate_waves", 1)                            # rounded up to 4
        assert deflate_checked(codec, head, 1, "deflate_waves = 1") == want_head
    finally:
        codec.set_param("deflate_waves", 0)
    assert len(got) == len(want)
    if got != want:
        sizes = [bsize for _, _, _, bsize in R.bgzf_payloads(want)]
        at = next(k for k in range(len(want)) if got[k] != want[k])
        assert False, "block %d differs" % next(k for k in range(len(sizes)) if sum(sizes[:k + 1]) > at)
    same_start = dc.repeated_preamble_blocks(16)
    want = deflate_checked(codec, same_start, 1, "blocks that begin alike, default sizing")
    codec.set_param("deflate_waves", 4)
    try:
        got = deflate_checked(codec, same_start, 1, "blocks that begin alike, deflate_waves = 4")
    finally:
        codec.set_param("deflate_waves", 0)
    assert got == want
    for blocks in R.walk_bgzf(got)[:-1]:
        assert all(isinstance(t, int) for t in blocks[0].tokens[:120]) and blocks[0].data[:60] == blocks[0].data[60:120]
    with pytest.raises(lib.BrambleError):
        codec.set_param("deflate_waves", -1)


@pytest.mark.parametrize("dynamic", [1, 0])
def test_random_streams_deflate_and_read_back(codec, dynamic):
    """60 streams of the inflate fuzz's mixtures (DEFLATE_FUZZ_SEED: another seed per soak run) through zlib, gzip and k_inflate;
    the five smallest token by token."""
    streams = list(dc.fuzz_streams())
    smallest = sorted(len(d) for _, d, _ in streams)[4]
    for label, data, exp in streams:
        raw = deflate_checked(codec, data, dynamic, label)
        if len(data) <= smallest:
            tokens_checked(raw, dynamic, label)


def test_the_matcher_finds_the_projected_streams_repeats(codec):
    """The record stream of test_device_deflate_compresses_projected_stream: its first block holds more matched bytes than
    literal bytes, and the per-block codes beat the fixed code."""
    ann = synth.Annotation("G", n_genes=1500, n_refs=3)
    b = ann.reads(8000, "pe", with_records=1)
    stream, roff, rlen = synth.Annotation.frame_records(b)
    idx = lib.Index(ann.as_dict(), device=0)
    ctx = lib.Context(idx)
    plain, _ = ctx.project_bam_bundle(lib.make_config(), stream, roff, rlen, np.arange(3, dtype=np.int32))
    plain = plain.tobytes()
    dyn, fix = deflate_checked(ctx, plain, 1, "dynamic"), deflate_checked(ctx, plain, 0, "fixed")
    first = R.bgzf_payloads(dyn)[0]
    (blk,) = R.inflate_exact(first[0])
    matched = sum(t[0] for t in blk.matches())
    print("projected stream of %d bytes: dynamic %.3f, fixed %.3f of the input; first block: %d matched bytes, %d literals"
          % (len(plain), len(dyn) / len(plain), len(fix) / len(plain), matched, len(blk.data) - matched))
    assert len(dyn) < len(fix) and len(dyn) < 0.5 * len(plain)
    assert matched > len(blk.data) - matched
    ctx.close()
    idx.close()

"""k_inflate on hand-built DEFLATE streams, code by code: the table of tests/inflate_cases.py (written token by token with
tests/deflate_write.py, each case pinned to what its name says in tests/test_inflate_cases_cpu.py) against zlib's bytes.
Codes of every length at every bit of the decode buffer and of the input ring, matches on both sides of the output window's
edge, the largest blocks, legal streams no encoder writes, every refusal by name, and a call long enough that every wave
takes several blocks of different codes one after the other."""
import numpy as np
import pytest
import torch

from bramble_amd import lib
from tests import inflate_cases as ic

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    idx = lib.Index({"refnames": ["chr1"], "transcripts": [{"id": "t", "ref_id": 0, "strand": "+", "exons": [[10, 50]]}]}, device=0)
    c = lib.Context(idx)
    yield c
    c.close(); idx.close()


@pytest.fixture(scope="module")
def zlib_bytes():
    """what zlib makes of every valid payload (the reference: computed once)"""
    out = {}
    for c in ic.of_class("valid"):
        data, eof, rest = ic.zlib_inflate(c.payload)
        assert eof and not rest
        out[c.name] = data
    return out


def table_of(cases):
    """(source bytes, block table, where each case's bytes go) of a call that holds these cases in this order: BGZF blocks as
    they are, the cases no frame holds as bare payloads; the table is made here, entry by entry (bgzf_scan's is compared with
    it in test_valid_cases_in_one_call)"""
    src, table, at, total = [], np.zeros(len(cases), dtype=lib.BGZF_BLOCK), 0, 0
    for k, c in enumerate(cases):
        raw = c.raw if c.raw is not None else c.direct()
        table[k] = (at + (12 + c.xlen if c.raw is not None else 0), total, c.clen, c.isize, c.crc, 0)
        src.append(raw)
        at += len(raw)
        total += c.isize
    return b"".join(src), table


def inflate(ctx, cases):
    src, table = table_of(cases)
    out = ctx.bgzf_inflate_device(torch.from_numpy(np.frombuffer(src, dtype=np.uint8).copy()).to("cuda:0"), table)
    return out.cpu().numpy().tobytes(), table


def first_wrong(got, cases, table, want_of):
    """the names of the cases whose bytes differ"""
    bad = []
    for c, row in zip(cases, table):
        o = int(row["dst_off"])
        if got[o:o + c.isize] != want_of(c):
            bad.append(c.name)
    return bad


def probe_case():
    """a small valid stream with a bit of everything: what a context must still inflate after it refused something"""
    return next(c for c in ic.of_class("valid") if c.name.startswith("block sequence: 15-bit codes"))


def test_valid_cases_alone(ctx, zlib_bytes):
    wrong = []
    for c in ic.of_class("valid"):
        try:
            got, _ = inflate(ctx, [c])
        except lib.BrambleError:
            wrong.append(c.name + " (refused)")
            continue
        if got != zlib_bytes[c.name]:
            wrong.append(c.name)
    assert not wrong, wrong[:20]


def test_valid_cases_in_one_call(ctx, zlib_bytes):
    cases = ic.of_class("valid")
    got, table = inflate(ctx, cases)
    want = b"".join(zlib_bytes[c.name] for c in cases)
    assert got == want, first_wrong(got, cases, table, lambda c: zlib_bytes[c.name])[:20]
    # the scan's table of the framed ones is the one made by hand (two extra subfields in one of them)
    framed = [c for c in cases if c.raw is not None]
    src, by_hand = table_of(framed)
    scanned, consumed, total = lib.bgzf_scan(np.frombuffer(src, dtype=np.uint8))
    assert consumed == len(src) and total == sum(c.isize for c in framed)
    assert scanned.tobytes() == by_hand.tobytes()


def test_invalid_cases_are_refused_alone(ctx, zlib_bytes):
    probe = probe_case()
    accepted = []
    for c in ic.of_class("invalid"):
        try:
            inflate(ctx, [c])
            accepted.append(c.name)
        except lib.BrambleError:
            pass
        got, _ = inflate(ctx, [probe])
        assert got == zlib_bytes[probe.name], "the call after " + c.name
    assert not accepted, accepted


def test_invalid_case_in_the_middle_refuses_the_call(ctx, zlib_bytes):
    around = [c for c in ic.of_class("valid") if len(c.want) < 3000][:12]
    want = b"".join(zlib_bytes[c.name] for c in around)
    accepted = []
    for c in ic.of_class("invalid"):
        try:
            inflate(ctx, around[:6] + [c] + around[6:])
            accepted.append(c.name)
        except lib.BrambleError:
            pass
        got, _ = inflate(ctx, around)
        assert got == want, "the call after " + c.name
    assert not accepted, accepted


def test_lenient_cases_are_refused_or_right(ctx, zlib_bytes):
    """what zlib or the strict reader refuses and the kernel's header comment lets pass: either, but never other bytes"""
    probe = probe_case()
    around = [c for c in ic.of_class("valid") if len(c.want) < 3000][:12]
    for c in ic.of_class("lenient"):
        try:
            got, _ = inflate(ctx, [c])
            verdict = "accepted"
            assert got == c.want, c.name
        except lib.BrambleError:
            verdict = "refused"
        print("lenient verdict: %s: %s" % (c.name, verdict))
        got, _ = inflate(ctx, [probe])
        assert got == zlib_bytes[probe.name], "the call after " + c.name
        cases = around[:6] + [c] + around[6:]
        try:
            got, table = inflate(ctx, cases)
            assert verdict == "accepted" and not first_wrong(got, cases, table, lambda x: x.want), c.name
        except lib.BrambleError:
            assert verdict == "refused", c.name
        got, _ = inflate(ctx, around)
        assert got == b"".join(zlib_bytes[x.name] for x in around), "the call after " + c.name


def test_waves_take_block_after_block_of_different_codes(ctx, zlib_bytes):
    """A wave takes another block only when a call has more blocks than waves (20 per compute unit): four times that many, the
    valid table over and over in a shuffled order, so that tables, long-code limits, code lengths and the ring of one code are
    what the next block's decode starts on."""
    valid = ic.of_class("valid")
    n = 4 * 20 * torch.cuda.get_device_properties(0).multi_processor_count
    order = np.random.RandomState(31).permutation(np.arange(n) % len(valid))
    cases = [valid[i] for i in order]
    assert n >= 4 * 20 * torch.cuda.get_device_properties(0).multi_processor_count and len(set(order.tolist())) == len(valid)
    got, table = inflate(ctx, cases)
    assert len(got) == sum(c.isize for c in cases)
    if got != b"".join(zlib_bytes[c.name] for c in cases):
        bad = first_wrong(got, cases, table, lambda c: zlib_bytes[c.name])
        raise AssertionError("%d of %d blocks differ: %s" % (len(bad), n, sorted(set(bad))[:20]))

"""The SAM text reader (k_sam_measure, k_sam_emit, the host's patch list) on generated input, through lib.SamReader alone:
float literals bit for bit against Python's float() cast to float32 (both sides of every limit of the device's exact path, the
patch list's regrowth with its second emit pass), the device's %g formatter and the reader against each other, a grammar of
valid lines byte for byte against tests/test_sam_cpu.py::encode_sam (whole and in pieces), and malformed lines against the
validator of tests/sam_cases.py.  The generators, the references and what is left out (an i tag spelled -0) are in
tests/sam_cases.py; tests/test_sam_cases_cpu.py checks them without a GPU."""
import numpy as np
import pytest

from bramble_amd import lib
from tests import bamio
from tests import sam_cases as sc
from tests.test_cg_tag_cpu import ANN
from tests.test_gpu_sam_out import NAMES, float_records, fmt
from tests.test_sam_cpu import encode_line, encode_sam

pytestmark = pytest.mark.gpu


def read_all(header, text):
    r = lib.SamReader(header)
    try:
        got = r.next(text, True)
    finally:
        r.close()
    assert got["consumed"] == len(text)
    return got


def assert_floats(stream, texts):
    got = sc.float_bits(stream)
    bad, n_bad = sc.float_mismatches(got, sc.float_ref_bits(texts), texts)
    assert n_bad == 0, "%d of %d differ; (literal, device bits, reference bits): %r" % (n_bad, len(texts), bad)


# ---- 1. float literals ------------------------------------------------------------------------------------------------------
def test_float_literals_bit_for_bit():
    fam = sc.float_families()
    text, order = sc.float_text(fam)
    on = sum(sc.on_fast_path(t) for t in order)
    print("float literals: %d in %d lines, %d on the device's path, %d off it" % (len(order), text.count(b"\n"), on, len(order) - on))
    assert len(order) >= 200000 and on >= 0.3 * len(order) and len(order) - on >= 0.3 * len(order)
    got = read_all(sc.FLOAT_HEADER, text)
    assert got["n"] == text.count(b"\n") and got["n_unmapped"] == 0
    assert_floats(got["stream"], order)


def test_float_patch_list_regrowth_and_second_call():
    """more floats off the device's path in one call than the patch list's first 4096 entries: the list is regrown and the
    emit pass runs again; the next call on the same reader patches its own few"""
    first, second = sc.off_path_literals(5000, 1), sc.off_path_literals(7, 2) + ["1e-45", "inf"]
    mixed = [t for k, t in enumerate(first) for t in ((t, "0.5") if k % 50 == 0 else (t,))]   # exact ones among them
    a = sc.FLOAT_LINE % ("a", 10) + "\tXb:B:f," + ",".join(mixed[:3000]) + "".join("\tX%d:f:%s" % (k % 10, t) for k, t in enumerate(mixed[3000:])) + "\n"
    b = sc.FLOAT_LINE % ("b", 11) + "\tXb:B:f," + ",".join(second) + "\n"
    c = sc.FLOAT_LINE % ("c", 12) + "\tXc:f:" + second[0] + "\n"
    r = lib.SamReader(sc.FLOAT_HEADER)
    try:
        g1 = r.next((a + b).encode(), False)   # (the last read name waits for the next call)
        assert g1["n"] == 1 and g1["consumed"] == len(a)
        assert_floats(g1["stream"], mixed)
        g2 = r.next((b + c).encode(), True)
        assert g2["n"] == 2 and g2["consumed"] == len(b + c)
        assert_floats(g2["stream"], second + second[:1])
    finally:
        r.close()


# ---- 2. the formatter and the reader against each other -----------------------------------------------------------------------
def test_floats_round_trip_through_formatter_and_reader():
    specials = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001,
                         0x00000001, 0x80000001, 0x007fffff, 0x00800000, 0x7f7fffff, 0xff7fffff, 0x3f800000], dtype=np.uint32)
    ties = np.array([123456.5, 123457.5, 1234565, 999999.5, 1e-45, 0.0001, 0.00001, 99999.95, 999999, 1e6, 1e-5, 9.999995e-5,
                     0.5, 2.5, 1e38, 3.4028235e38, 1.17549435e-38, 100000, 123456, 0.1, 1.0 / 3], dtype=np.float32).view(np.uint32)
    rng = np.random.RandomState(77)
    bits = np.concatenate([specials, ties, rng.randint(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)])
    idx = lib.Index(ANN, device=0)
    ctx = lib.Context(idx)
    try:
        ctx.set_sam_refs(NAMES)
        text = fmt(ctx, bamio.frame(float_records(bits, per=50000)))
    finally:
        ctx.close()
        idx.close()
    assert text.count(b",") == bits.size
    want = ["%g" % float(v) for v in bits.view(np.float32)]
    got = read_all("".join("@SQ\tSN:%s\tLN:1000\n" % n for n in NAMES), text)
    assert got["n"] == (bits.size + 49999) // 50000
    assert_floats(got["stream"], want)


# ---- 3. valid lines -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def valid():
    text, names = sc.valid_text()
    with np.errstate(over="ignore"):
        exp, n_un, _ = encode_sam(text, names)
    return text, sc.header_of(names), names, exp, n_un


def first_difference(got, exp):
    a, b = sc.records(got), sc.records(exp)
    for k, (x, y) in enumerate(zip(a, b)):
        if x != y:
            at = next(i for i in range(min(len(x), len(y))) if x[i] != y[i]) if x[:min(len(x), len(y))] != y[:min(len(x), len(y))] else min(len(x), len(y))
            return "record %d (%r): %d / %d bytes, first difference at byte %d: %r / %r" % (k, x[32:32 + x[8] - 1][:40], len(x), len(y), at,
                                                                                       x[at:at + 16], y[at:at + 16])
    return "%d / %d records" % (len(a), len(b))


def test_valid_lines_byte_for_byte(valid):
    text, header, names, exp, n_un = valid
    missing = sc.missing_coverage(sc.coverage(text, names))
    assert missing == [], missing
    got = read_all(header, text)
    print("valid lines: %d, %d unmapped, %d bytes of text" % (len(sc.split_lines(text)), n_un, len(text)))
    assert got["n_unmapped"] == n_un and got["n"] == len(sc.split_lines(text)) - n_un
    assert np.array_equal(got["stream"], exp), first_difference(got["stream"], exp)


@pytest.mark.parametrize("piece", [997, 4099, 65537])
def test_valid_lines_in_pieces(valid, piece):
    text, header, names, exp, n_un = valid
    r = lib.SamReader(header)
    try:
        parts, un, pos, end, calls = [], 0, 0, min(piece, len(text)), 0
        while True:
            last = end >= len(text)
            got = r.next(text[pos:end], last)
            calls += 1
            un += got["n_unmapped"]
            if got["n"]:
                parts.append(got["stream"])
            if got["consumed"] == 0 and not last:
                end = min(len(text), end + piece)
                continue
            pos += got["consumed"]
            if last:
                assert pos == len(text)
                break
            end = min(len(text), pos + piece)
    finally:
        r.close()
    print("pieces of %d: %d calls, %d bundles" % (piece, calls, len(parts)))
    name = lambda rec: rec[32:32 + rec[8] - 1]
    for a, b in zip(parts, parts[1:]):   # every bundle ends at a read-name change
        assert name(sc.records(a)[-1]) != name(sc.records(b)[0])
    cat = np.concatenate(parts)
    assert un == n_un and np.array_equal(cat, exp), first_difference(cat, exp)
    assert len(parts) > (1 if piece > 60000 else 50)


# ---- 4. malformed lines -------------------------------------------------------------------------------------------------------
def join(lines):
    return b"".join(l + b"\n" for l in lines)


@pytest.fixture(scope="module")
def block():
    lines = sc.valid_block()
    exp, n_un, _ = encode_sam(join(lines), sc.BLOCK_REFS)
    return lines, exp, n_un


def refused(r, text, last=True):
    with pytest.raises(lib.SamError) as e:
        r.next(text, last)
    return e.value


def test_malformed_lines_one_rule_each(block):
    good, exp, n_un = block
    cases = sc.malformed_cases()
    for name, lines, at, rule in cases:
        assert sc.first_error(lines) == (at, rule), name
        r = lib.SamReader(sc.BLOCK_HEADER)
        try:
            e = refused(r, join(lines))
        finally:
            r.close()   # the reader that refused is closed ...
        assert e.line == at, (name, e)
        if rule in sc.REASON_WORD:
            assert sc.REASON_WORD[rule] in e.reason, (name, e)
        got = read_all(sc.BLOCK_HEADER, join(good))   # ... and a fresh one reads the valid block
        assert got["n_unmapped"] == n_un and np.array_equal(got["stream"], exp), name
    print("malformed cases: %d" % len(cases))


def test_the_earlier_of_two_bad_lines_is_reported(block):
    good, _, _ = block
    base = good[0].split(b"\t")[:11]

    def bad(qname, field=None, value=None, tag=None, flag=None):
        f = [qname] + base[1:]
        if flag is not None:
            f[1] = flag
        if field is not None:
            f[field] = value
        return b"\t".join(f + ([tag] if tag is not None else []))

    cigar, flt, rng_, few = bad(b"x1", 5, b"5Q"), bad(b"x2", tag=b"XX:f:1.5x"), bad(b"x3", tag=b"XX:i:4294967296"), b"x4\t0\tchr1\t5"
    for first, second, word in ((cigar, flt, "CIGAR"), (flt, cigar, "float"), (rng_, few, "out of range"), (few, rng_, "fields"),
                                (bad(b"x5", tag=b"XX:f:1e", flag=b"4"), few, "float"),        # the earlier one is an unmapped line
                                (bad(b"x6", 5, b"5Q", flag=b"4"), flt, "CIGAR")):
        lines = good[:20] + [first] + good[20:30] + [second] + good[30:]
        assert sc.first_error(lines)[0] == 21
        r = lib.SamReader(sc.BLOCK_HEADER)
        try:
            e = refused(r, join(lines))
        finally:
            r.close()
        assert e.line == 21 and word in e.reason, (first, e)
    # both in the text's last read-name group, which a call that is not the last leaves for the next one
    g = good[-1].split(b"\t")[0]
    for last in (False, True):
        lines = good[:-1] + [bad(g, 5, b"5Q"), bad(g, tag=b"XX:f:--1"), good[-1]]
        r = lib.SamReader(sc.BLOCK_HEADER)
        try:
            e = refused(r, join(lines), last)
        finally:
            r.close()
        assert e.line == len(good) == sc.first_error(lines)[0] and "CIGAR" in e.reason, e


def test_bad_line_number_counts_from_the_start_of_a_chunked_feed(block):
    good, exp, _ = block
    tag, piece = b"\tXX:B:c,128", 997
    # where the calls cut the valid block: everything in front of the last mapped line a call holds whole (one read name a line)
    refs = {n: k for k, n in enumerate(sc.BLOCK_REFS)}
    mapped = [encode_line(l, refs)[1] for l in good]
    starts = [0]
    for l in good:
        starts.append(starts[-1] + len(l) + 1)
    pos, ends = 0, []
    for _ in range(2):
        whole = [k for k in range(len(good)) if starts[k] >= pos and starts[k + 1] <= pos + piece]
        ends.append(pos + piece)
        pos = starts[[k for k in whole if mapped[k]][-1]]
    # the first line that the second call does not hold whole and the third one does, the tag included
    at = next(k for k in range(len(good)) if starts[k + 1] > ends[1] and starts[k] >= pos and starts[k + 1] + len(tag) <= pos + piece)
    lines = good[:at] + [good[at] + tag] + good[at + 1:]
    assert sc.first_error(lines) == (at + 1, "out of range")
    text = join(lines)
    r = lib.SamReader(sc.BLOCK_HEADER)
    try:
        pos, calls, parts = 0, 0, []
        with pytest.raises(lib.SamError) as e:
            while True:
                end = min(len(text), pos + piece)
                got = r.next(text[pos:end], end >= len(text))
                calls += 1
                assert got["consumed"] > 0
                parts.append(got["stream"])
                pos += got["consumed"]
        assert calls == 2 and e.value.line == at + 1 and "out of range" in e.value.reason, (calls, e.value)
        done = np.concatenate(parts)
        assert np.array_equal(done, exp[:done.size])   # what the first two calls gave is the valid lines' records
    finally:
        r.close()

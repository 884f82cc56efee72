"""The generators and references of tests/sam_cases.py on the CPU: they are deterministic, the float list has the mix the GPU
tests need, the tests' encoder takes every generated line, the generated text holds every case tests/test_gpu_sam_fuzz.py
claims to reach, and the validator finds exactly the planted line of every malformed case."""
import struct

import numpy as np
import pytest

from tests import sam_cases as sc
from tests.test_sam_cpu import encode_line, encode_sam


@pytest.fixture(scope="module")
def families():
    return sc.float_families()


@pytest.fixture(scope="module")
def valid():
    return sc.valid_text()


def test_generators_are_deterministic(families, valid):
    again = sc.float_families()
    assert list(again) == list(families) and all(again[k] == families[k] for k in families)
    assert sc.float_text(again) == sc.float_text(families)
    assert sc.valid_text() == valid
    assert sc.valid_text(seed=12, n_random=50)[0] != sc.valid_text(seed=11, n_random=50)[0]
    assert sc.malformed_cases() == sc.malformed_cases() and sc.valid_block() == sc.valid_block()
    assert sc.off_path_literals(50, 1) == sc.off_path_literals(50, 1)


def test_float_list_mix(families):
    text, order = sc.float_text(families)
    n = len(order)
    on = sum(sc.on_fast_path(t) for t in order)
    print("float literals: %d in %d lines, %d on the device's path, %d off it" % (n, text.count(b"\n"), on, n - on))
    for k, v in families.items():
        print("  %-28s %7d literals, %7d on the path" % (k, len(v), sum(sc.on_fast_path(t) for t in v)))
    assert n >= 200000 and 200 <= text.count(b"\n") <= 900
    assert on >= 0.3 * n and n - on >= 0.3 * n
    assert not any("\t" in t or "," in t or "\n" in t for t in order)
    # both sides of each limit of the path
    side = lambda ts: {sc.on_fast_path(t) for t in ts}
    assert side(["9007199254740992", "9007199254740993"]) == {True, False}
    assert side(["1234567890123456789e-22", "1234567890123456789e-23"]) == {False}   # 19 digits, but past 2^53
    assert side(["999999999999999e-22", "999999999999999e-23"]) == {True, False}
    assert sc.on_fast_path("9007199254740992e22") and not sc.on_fast_path("9007199254740992e23")
    assert sc.on_fast_path("0.0000000000000000000001") and not sc.on_fast_path("0.00000000000000000000001")
    assert sc.on_fast_path("0e999999999") and sc.on_fast_path("000.000100") and sc.on_fast_path("1E+0000000000000000000022")
    assert not sc.on_fast_path("inf") and not sc.on_fast_path(" 1.5") and not sc.on_fast_path("0x1p-149") and not sc.on_fast_path("1e-45")
    # the reference: double first, then float
    ref = sc.float_ref_bits(["16777217", "1.0000000596046448", "3.4028235677973366e38", "3.4028235677973365e38", "7e-46", "7.1e-46", "0x1.ffffffp127",
                             "-0", "1e-45", "0X10"])
    assert [int(b) for b in ref] == [0x4b800000, 0x3f800000, 0x7f800000, 0x7f800000, 0, 1, 0x7f800000, 0x80000000, 1, 0x41800000]
    # every literal of the list has a reference value, and the stream reader finds them in the encoder's own records
    want = sc.float_ref_bits(order)
    assert want.shape == (n,)
    few = b"\n".join(text.split(b"\n")[::40]) + b"\n"
    few_order = [t for l in few.decode().split("\n") if l for f in l.split("\t")[11:] for t in (f[7:].split(",") if f[3] == "B" else [f[5:]])]
    with np.errstate(over="ignore"):
        got = sc.float_bits(encode_sam(few, ["chr1"])[0])
    assert sc.float_mismatches(got, sc.float_ref_bits(few_order), few_order) == ([], 0)


def test_encoder_takes_every_valid_line_and_the_text_reaches_every_case(valid):
    text, names = valid
    lines = sc.split_lines(text)
    assert 2000 <= len(lines) <= 6000 and len(names) == sc.N_REFS == len(set(names))
    assert sc.first_error(lines) is None
    stream, n_un, every = encode_sam(text, names)
    assert len(sc.records(every)) == len(lines) and 0 < n_un < len(lines) // 4
    missing = sc.missing_coverage(sc.coverage(text, names))
    assert missing == [], missing
    print("valid lines: %d (%d unmapped), %d bytes of text, %d bytes of records" % (len(lines), n_un, len(text), stream.size))
    # the reference names make the table probe and wrap: names pushed off their home slot, some of them past the table's end
    slots, sz = sc.table_slots(names)
    moved = [(h, k) for h, k in slots if h != k]
    assert sz == 2048 and len(moved) > 100 and sum(1 for h, k in moved if k < h) >= 2
    assert max((k - h) % sz for h, k in moved) >= 3
    assert {1, 200} <= {len(n) for n in names} and b"chr1" in names and b"chr10" in names and b"chr100" in names
    # the 16-bit bin past 2^29: the named case the encoder was mended for
    rec, mapped = encode_line(b"far\t0\tchr1\t2147483000\t9\t3M\t*\t0\t0\tAAA\tIII", {b"chr1": 0})
    assert mapped and struct.unpack_from("<H", rec, 14)[0] == (4681 + (2147482999 >> 14)) & 0xffff == 4680


def test_validator_finds_the_planted_line(families):
    block = sc.valid_block()
    assert len(block) == 50 and sc.first_error(block) is None
    assert len({l.split(b"\t")[0] for l in block}) == len(block) and max(len(l) for l in block) <= 120
    cases = sc.malformed_cases()
    assert len(cases) == 47
    for name, lines, at, rule in cases:
        assert sc.first_error(lines) == (at, rule), name
        assert sc.first_error(lines[:at - 1] + lines[at:]) is None, name
    rules = {c[3] for c in cases}
    assert set(sc.REASON_WORD) <= rules
    # what strtod takes whole is valid, and so is every generated literal
    for t in (b"XX:f: 1.5", b"XX:f:-inf", b"XX:f:NaN", b"XX:f:0x1.8p1", b"XX:f:nan(abc_1)", b"XX:f:5.", b"XX:f:.5e1", b"XX:B:f,infinity,0X10", b"XX:B:f",
              b"XX:B:c", b"XX:i:+0000000000000000000000000000005"):
        assert sc.line_rule(block[0] + b"\t" + t) is None, t
    for t in sc.float_text(families)[1][::97]:
        assert sc.line_rule(block[0] + b"\tXX:f:" + t.encode()) is None, t

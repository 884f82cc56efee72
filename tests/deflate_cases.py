"""Seeded payloads for the device's BGZF deflate (codec_kernels.hip: k_deflate_dynamic, k_deflate_fixed) and what the token
list of each must hold for the case to have tested anything.  No GPU and no test functions here: tests/test_deflate_cases_cpu.py
checks on the CPU that the cases mean what they say, tests/test_gpu_codec.py sends them through the encoder and reads the
blocks back with tests/deflate_ref.py.

Every generator yields (label, bytes, expectations); expectations is a dict:

  group        plants of one kind (same distance, same length and offset, same size) with eight different seeds share a group.
               The encoder's hash table is lossy (2048 slots, the last writer wins), so a single planted distance may go
               unseen; there the rule is that at least ONE plant of a group shows what the group expects (shows() below).
               The planted lengths and ends are chosen or built so that nothing overwrites their slot: every plant shows.
  dist         a match of exactly this distance starts inside the second copy of the seed
  token_at     (position, length, distance): a match token of exactly this length and distance starts at this position
  end_match    the last token is a match that ends on the payload's last byte
  one_match    the block holds exactly one match (one distance symbol: the incomplete one-bit distance code)
  no_match     the block holds literals only (thirty distance code lengths of zero)
  min_matches  at least this many matches
  hist         the byte histogram the payload was built from (256 counts; end-of-block is not in it), for the code-length
               cases

What the encoder cannot do by its documented design carries no expectation: the 128 positions of one parse step are looked
up before any of them enters the table, so a match never reaches back to a position of its own step.  Seeds planted at a
distance below 128 are therefore only round-tripped, and so are the payloads of 130 and 131 bytes of matches_to_the_end():
all of the 128 positions of their first step are literals, and the 2 or 3 bytes after it are too short for a match."""
import os

import numpy as np

PAYLOAD = 57344          # DEFLATE_PAYLOAD of kernels.h: input bytes per BGZF block
MIN_MATCH, MAX_MATCH, MAX_DIST = 4, 258, 32768   # the encoder's shortest match; RFC 1951's longest match and distance
STEP = 128               # positions per parse step
N_SEEDS = 8

LENGTHS = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 257, 258,
           259, 300, 516, 1000]
OFFSETS = [0, 1, 62, 63, 64, 65, 126, 127]
# distance codes from 128 up: code 2k + 2 starts at 2^k + 1, code 2k + 3 at 3 * 2^(k-1) + 1; the distance before each is the
# last of the code below (all extra bits set)
DIST_EDGES = sorted(set([128, 129, 32767, 32768, 32769] + [e + s for k in range(7, 15) for e in (2 ** k, 3 * 2 ** (k - 1)) for s in (0, 1)]))
DIST_NEAR = [5, 9, 17, 33, 65, 97, 127]     # below one parse step: no expectation
END_SIZES = [130, 131, 132, 133, 1000, 1001, 1002, 1003, PAYLOAD]
SIZES = sorted(set(list(range(1, 10)) + [63, 64, 65] + list(range(127, 133)) + [895, 896, 897, 1791, 1792, 1793]
                   + [PAYLOAD - 1, PAYLOAD, PAYLOAD + 1, PAYLOAD + 895, PAYLOAD + 896, PAYLOAD + 897, 2 * PAYLOAD - 1, 2 * PAYLOAD, 2 * PAYLOAD + 1]))


def _absent(*arrays):
    """byte values that occur in none of the arrays, ascending"""
    seen = np.zeros(256, dtype=bool)
    for a in arrays:
        seen[np.asarray(a, dtype=np.uint8)] = True
    return [v for v in range(256) if not seen[v]]


def _random_without(rng, n, banned):
    ok = np.array([v for v in range(256) if v not in banned], dtype=np.uint8)
    return ok[rng.randint(0, len(ok), size=n)]


# ---- planted matches ------------------------------------------------------------------------------------------------------
def plant_distance(d, seed):
    """seed R at 0, a filler of one repeated byte (one hash slot, so that R's slots stay alive), R again at d"""
    rng = np.random.RandomState(8191 * d + seed)
    r = rng.randint(0, 256, size=min(300, d - 4)).astype(np.uint8)
    f = _absent(r)[0]
    data = np.concatenate([r, np.full(d - len(r), f, dtype=np.uint8), r])
    return data.tobytes(), len(r)


def planted_distances():
    for d in DIST_NEAR + DIST_EDGES:
        for seed in range(N_SEEDS):
            data, rlen = plant_distance(d, seed)
            exp = {"group": ("distance", d), "copy": (d, rlen)}
            if STEP <= d <= MAX_DIST:
                exp["dist"] = d
            yield "seed again at distance %d, plant %d" % (d, seed), data, exp


def plant_length(length, offset, seed, dist=4096):
    """A stretch S of `length` random bytes at s0, its copy at s0 + dist, both inside a filler of one repeated byte; the bytes
    before the two differ, and the bytes after them.  s0 = offset mod 128: the copy starts in that lane of a half-round."""
    rng = np.random.RandomState((length * 131 + offset) * 17 + seed)
    f = int(rng.randint(0, 256))
    a, b, x, y = [int(v) for v in rng.permutation([v for v in range(256) if v != f])[:4]]
    s = _random_without(rng, length, {f})
    s0 = 2 * STEP + offset
    fill = lambda n: np.full(n, f, dtype=np.uint8)
    one = lambda v: np.array([v], dtype=np.uint8)
    data = np.concatenate([fill(s0 - 1), one(a), s, one(x), fill(dist - length - 2), one(b), s, one(y), fill(32)])
    return data.tobytes(), s0 + dist


def table_slots(data):
    """the encoder's table index of every position's four bytes: (little-endian word * 2654435761 mod 2^32) >> (32 - HASH_BITS),
    HASH_BITS = 11 (parse_step in codec_kernels.hip); the last three positions have none"""
    a = np.frombuffer(data, dtype=np.uint8).astype(np.uint64)
    w = a[:-3] | (a[1:-2] << np.uint64(8)) | (a[2:-1] << np.uint64(16)) | (a[3:] << np.uint64(24))
    return ((w * np.uint64(2654435761)) & np.uint64(0xffffffff)) >> np.uint64(21)


def slot_kept(data, src, p):
    """No other position from the first of src's parse step to the last before p's step shares src's table slot: whichever
    lane wins a clash within a step, the table still holds src when the step of p looks it up."""
    slots = table_slots(data)
    lo, hi = src // STEP * STEP, p // STEP * STEP
    return int((slots[lo:hi] == slots[src]).sum()) == 1


def planted_lengths(offsets=OFFSETS):
    """Eight plants per length and offset, each the next seed whose stretch keeps its table slot until the copy is looked up
    (slot_kept: about one seed in L / 2048 does not): every one of them must be found."""
    for length in LENGTHS:
        for offset in offsets:
            seed, k = 0, 0
            while k < N_SEEDS:
                data, p = plant_length(length, offset, seed)
                seed += 1
                if not slot_kept(data, p - 4096, p):
                    continue
                yield ("a copy of %d bytes at %d mod 128, plant %d" % (length, offset, k), data,
                       {"group": ("length", length, offset), "token_at": (p, min(length, MAX_MATCH), 4096), "copy": (p, length)})
                k += 1


def plant_end(n, seed):
    """64 random bytes (within 30000 bytes of the end: a filler comes first in a long payload), a filler, then the payload's last
    k bytes (k = 5, 10, .., 40 by the seed) copy a stretch of the 64"""
    rng = np.random.RandomState(n * 29 + seed)
    k = 5 * (seed % 8 + 1)
    f = int(rng.randint(0, 256))
    r = _random_without(rng, 64, {f})
    a = int(rng.randint(1, 64 - k + 1))
    b = [v for v in range(256) if v != f and v != r[a - 1]][int(rng.randint(0, 254))]
    pre = max(0, n - 30000)
    data = np.concatenate([np.full(pre, f, dtype=np.uint8), r, np.full(n - pre - k - 1 - 64, f, dtype=np.uint8), np.array([b], dtype=np.uint8), r[a:a + k]])
    assert len(data) == n
    return data.tobytes(), k


def matches_to_the_end():
    for n in END_SIZES:
        for seed in range(N_SEEDS):
            data, k = plant_end(n, seed)
            exp = {"group": ("end", n), "copy": (n - k, k)}
            if n - STEP >= MIN_MATCH:          # (see the module's docstring)
                exp["end_match"] = n
            yield "the last %d of %d bytes copy an earlier stretch, plant %d" % (k, n, seed), data, exp


# ---- code lengths ---------------------------------------------------------------------------------------------------------
def from_histogram(hist, seed):
    hist = np.asarray(hist, dtype=np.int64)
    data = np.repeat(np.arange(256, dtype=np.uint8), hist)
    np.random.RandomState(seed).shuffle(data)
    return data.tobytes()


def fibonacci_histogram():
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= PAYLOAD:
        fib.append(fib[-1] + fib[-2])
    return fib[1:] + [0] * (257 - len(fib))      # (end-of-block is the ladder's first 1)


def code_length_cases():
    rng = np.random.RandomState(77)

    def case(label, hist, seed, **exp):
        hist = [int(v) for v in hist]
        assert len(hist) == 256 and 0 < sum(hist) <= PAYLOAD
        exp["hist"] = hist
        return label, from_histogram(hist, seed), exp

    yield case("Fibonacci ladder (Huffman depth above 15)", fibonacci_histogram(), 1)
    # with end-of-block the frequencies are 2^14 .. 2, 1, 1 of 2^15: the Shannon lengths already are a complete code
    yield case("exact powers of two", [1 << (14 - k) for k in range(15)] + [0] * 241, 2)
    # 3 * 2^13 .. 3 of 3 * 2^14 take 1 .. 14 bits, which leaves 2^-14; two literals and end-of-block of frequency 1 want 16 bits
    # and get 15: three halves of the rest, the one histogram family whose Kraft sum starts above one
    yield case("three times powers of two and two rare bytes (Kraft above one at 15 bits)", [3 << (13 - k) for k in range(14)] + [1, 1] + [0] * 240, 3)
    below = [PAYLOAD // 256 - 1] * 256
    below[200] += PAYLOAD - sum(below)
    yield case("255 bytes just below 1/256 and one above (the maximal slack)", below, 4)
    for k in (1, 2, 3, 63, 64, 65, 127, 128, 254):
        h = [0] * 256
        for v in rng.permutation(255)[:k]:
            h[int(v)] = 1
        h[255] = 6000 - k
        yield case("%d bytes of frequency 1 beside one heavy byte" % k, h, 10 + k)
    h = [0] * 256; h[3] = h[250] = 2048
    yield case("two bytes, evenly", h, 5)
    h = [0] * 256; h[0] = 4000; h[1] = 4
    yield case("two bytes, one of them rare", h, 6)
    h = [0] * 256; h[65] = 100
    yield case("one byte, 100 times (within one parse step: literals only)", h, 7, no_match=True)
    h = [0] * 256; h[65] = 5000
    yield case("one byte, 5000 times (a run of matches)", h, 8, min_matches=10)
    yield case("uniform over 256 (the largest literal-only block)", [PAYLOAD // 256] * 256, 9)
    yield case("uniform over 256, short", [3] * 256, 19, no_match=True)
    # exactly one match: the distance code is the single one-bit code
    r = np.random.RandomState(78).permutation(256).astype(np.uint8)
    data = np.concatenate([r[:200], r[200:250], r[40:80], r[250:256]])
    yield "one match among distinct bytes (one distance symbol)", data.tobytes(), {"one_match": True, "hist": np.bincount(data, minlength=256).tolist()}
    # the widest alphabet: literals of all 256 values, length-4 matches at far distances of every code (13 extra bits)
    base = np.random.RandomState(79).randint(0, 256, size=PAYLOAD).astype(np.uint8)
    r2 = np.random.RandomState(80)
    for p in range(2048, PAYLOAD - 8, 9):
        back = int(r2.randint(STEP, min(p, MAX_DIST) + 1))
        base[p:p + 4] = base[p - back:p - back + 4]
    yield ("length-4 matches at far distances among literals of all 256 values", base.tobytes(),
           {"min_matches": 500, "hist": np.bincount(base, minlength=256).tolist()})


# ---- sizes ----------------------------------------------------------------------------------------------------------------
def size_cases():
    rng = np.random.RandomState(123)
    for n in SIZES:
        yield "%d random bytes" % n, rng.randint(0, 256, size=n).astype(np.uint8).tobytes(), {}
        period = rng.randint(0, 256, size=7).astype(np.uint8)
        yield "%d bytes of period 7" % n, np.tile(period, n // 7 + 1)[:n].tobytes(), {}


# ---- many unlike blocks for one wave ----------------------------------------------------------------------------------------
def unlike_blocks(n_blocks=64):
    """n_blocks - 1 full blocks whose neighbours differ as much as possible -- random, zeros, text, two letters, far repeats, and
    again -- and a last block of one byte"""
    rng = np.random.RandomState(4242)
    text = b"@read%07d\tACGTACGTTTGACCA\t+\tIIIIHHHGGFF###\n"
    out = []
    for k in range(n_blocks - 1):
        kind = k % 5
        if kind == 0: blk = rng.randint(0, 256, size=PAYLOAD).astype(np.uint8)
        elif kind == 1: blk = np.zeros(PAYLOAD, dtype=np.uint8)
        elif kind == 2: blk = np.frombuffer((text * (PAYLOAD // len(text) + 1))[:PAYLOAD], dtype=np.uint8)
        elif kind == 3: blk = ((rng.rand(PAYLOAD) < 0.9).astype(np.uint8) * 3 + 64)
        else: blk = np.tile(rng.randint(0, 256, size=20000).astype(np.uint8), 3)[:PAYLOAD]
        out.append(blk)
    out.append(np.array([0x7f], dtype=np.uint8))
    return np.concatenate(out).tobytes()


def repeated_preamble_blocks(n_blocks=16):
    """n_blocks - 1 full blocks that begin alike -- 60 random bytes twice, inside the first parse step -- and go on with one
    repeated byte each (another one per block: one table slot), and a last block of one byte.  Within a step nothing is
    looked up that the step itself has put into the table, so the second 60 are literals.  A table that a wave carried over
    from its last block would still hold them, at the very positions that look them up."""
    rng = np.random.RandomState(777)
    r = rng.randint(0, 256, size=60).astype(np.uint8)
    fillers = _absent(r)
    out = []
    for k in range(n_blocks - 1):
        out += [r, r, np.full(PAYLOAD - 120, fillers[k % len(fillers)], dtype=np.uint8)]
    out.append(np.array([0x7f], dtype=np.uint8))
    return np.concatenate(out).tobytes()


# ---- fuzz -------------------------------------------------------------------------------------------------------------------
def fuzz_streams(n_streams=60, seed=None):
    """Streams of 1 byte to 400 KB from the mixtures of tests/test_gpu_inflate.py::test_random_streams_of_every_make.  The seed
    comes from DEFLATE_FUZZ_SEED (soak runs: another seed per run)."""
    rng = np.random.RandomState(int(os.environ.get("DEFLATE_FUZZ_SEED", 20261020)) if seed is None else seed)

    def piece(n):
        kind = rng.randint(0, 8)
        if kind == 0: return np.minimum(rng.geometric(0.02 + 0.5 * rng.rand(), size=n) - 1, 255).astype(np.uint8)
        if kind == 1: return (rng.randint(0, rng.randint(2, 20), size=n) * rng.randint(1, 13) + rng.randint(0, 40)).astype(np.uint8)
        if kind == 2: return np.tile(rng.randint(0, 256, size=rng.randint(1, 300)).astype(np.uint8), n // 2 + 1)[:n]
        if kind == 3: return rng.randint(0, 256, size=n).astype(np.uint8)
        if kind == 4: return np.full(n, rng.randint(0, 256), dtype=np.uint8)
        if kind == 5: return np.where(rng.rand(n) < 0.02 + 0.3 * rng.rand(), rng.randint(0, 256, size=n), rng.randint(0, 256)).astype(np.uint8)
        if kind == 6:   # a sawtooth with noise: matches at one distance, broken up
            p = rng.randint(3, 2000)
            base = np.tile(rng.randint(0, 256, size=p).astype(np.uint8), n // p + 2)[:n].copy()
            hits = rng.rand(n) < 0.01 * rng.randint(1, 20)
            base[hits] = rng.randint(0, 256, size=int(hits.sum()))
            return base
        return np.frombuffer((b"@r%06d/1\tchr%d\t%d\t60\t100M\n" % (rng.randint(0, 10**6), rng.randint(1, 23), rng.randint(0, 10**8))) * (n // 30 + 1), dtype=np.uint8)[:n]

    for k in range(n_streams):
        parts, size = [], int(rng.randint(1, 400_000) if k % 7 else rng.randint(1, 300))
        while sum(len(p) for p in parts) < size:
            parts.append(piece(int(rng.randint(1, 40_000))))
        if len(parts) > 2 and rng.rand() < 0.5:   # something from far back, again
            parts.append(np.concatenate(parts)[:int(rng.randint(1, 70_000))])
        yield "fuzz stream %d, %d bytes" % (k, size), np.concatenate(parts)[:size].tobytes(), {}


# ---- reading the expectations ---------------------------------------------------------------------------------------------
def shows(exp, tokens, n):
    """Does this token list (of one payload of n bytes, positions from its start) hold what `exp` expects?  [] or the list of
    what is missing."""
    matches = [t for t in tokens if not isinstance(t, int)]
    missing = []
    if "dist" in exp:
        lo, rlen = exp["copy"]
        if not any(d == exp["dist"] and lo <= pos < lo + rlen for (l, d, pos) in matches):
            missing.append("no match at distance %d inside the copy" % exp["dist"])
    if "token_at" in exp:
        pos, length, dist = exp["token_at"]
        if (length, dist, pos) not in matches:
            missing.append("no match of length %d, distance %d at %d (there: %r)" % (length, dist, pos, [m for m in matches if m[2] == pos]))
    if "end_match" in exp:
        last = tokens[-1] if tokens else None
        if last is None or isinstance(last, int) or last[2] + last[0] != n:
            missing.append("the last token %r is no match that ends at %d" % (last, n))
    if exp.get("one_match") and len(matches) != 1:
        missing.append("%d matches, not one" % len(matches))
    if exp.get("no_match") and matches:
        missing.append("%d matches, not none" % len(matches))
    if len(matches) < exp.get("min_matches", 0):
        missing.append("%d matches, fewer than %d" % (len(matches), exp["min_matches"]))
    return missing


def wrong_tokens(exp, tokens):
    """What no plant may show, found or not: a match that starts on a planted copy of known length at the planted distance
    but has another length."""
    if "token_at" not in exp:
        return []
    pos, length, dist = exp["token_at"]
    return [m for m in tokens if not isinstance(m, int) and m[2] == pos and m[1] == dist and m[0] != length]


def groups_missing(results):
    """results: [(exp, missing)] of many payloads -> {group: [missing of every plant]} for the groups in which NO plant showed
    what it expects; payloads without a group count alone."""
    by = {}
    for k, (exp, missing) in enumerate(results):
        by.setdefault(exp.get("group", ("alone", k)), []).append(missing)
    return {g: ms for g, ms in by.items() if all(ms)}

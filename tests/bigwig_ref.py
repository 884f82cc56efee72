"""A bigWig reader for the tests, written from the layout in include/bramble_amd.h (br_coverage_bigwig) with struct and zlib only.
It walks the header, both kinds of tree in full -- node padding, key order, bounds containment and the root-first, left-to-right
placement of the nodes at every level -- answers a query by descending the R-tree, and decodes sections and zoom blocks
(zlib.decompress checks every Adler-32).  Every check is an assert: a file it reads to the end is well formed."""
import struct
import zlib

import numpy as np

BIGWIG_MAGIC, CHROM_MAGIC, RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
ITEM = np.dtype([("start", "<u4"), ("end", "<u4"), ("value", "<f4")])
ZOOM = np.dtype([("chrom", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid", "<u4"), ("min", "<f4"), ("max", "<f4"), ("sum", "<f4"),
                 ("sumsq", "<f4")])


def levels_of(n, block_size):
    """(blockSize of the header, items per level from the leaves up): a level over m items has ceil(m / bs) nodes, at least one"""
    bs = min(block_size, max(n, 1))
    items = [n]
    while max(-(-items[-1] // bs), 1) > 1:
        items.append(-(-items[-1] // bs))
    return bs, items


def header(data):
    f = struct.unpack_from("<IHHQQQHHQQIQ", data, 0)
    h = dict(zip(("magic", "version", "zoom_levels", "chrom_tree", "full_data", "full_index", "field_count", "defined_fields", "auto_sql",
                  "total_summary", "uncompress_buf", "extension"), f))
    assert h["magic"] == BIGWIG_MAGIC and h["version"] == 4 and (h["field_count"], h["defined_fields"], h["auto_sql"], h["extension"]) == (0, 0, 0, 0)
    assert struct.unpack_from("<I", data, len(data) - 4)[0] == BIGWIG_MAGIC
    h["zooms"] = []
    for k in range(h["zoom_levels"]):
        red, zero, d, i = struct.unpack_from("<IIQQ", data, 64 + 24 * k)
        assert zero == 0
        h["zooms"].append({"reduction": red, "data": d, "index": i})
    assert h["total_summary"] == 64 + 24 * h["zoom_levels"] and h["chrom_tree"] == h["total_summary"] + 40
    s = struct.unpack_from("<Qdddd", data, h["total_summary"])
    h["summary"] = dict(zip(("valid", "min", "max", "sum", "sumsq"), s))
    return h


def _nodes(data, at, bs, item_bytes, n_nodes):
    """the nodes of one level: [(is_leaf, [item bytes])], the padding of every node checked"""
    out = []
    for k in range(n_nodes):
        p = at + k * (4 + bs * item_bytes)
        leaf, zero, count = struct.unpack_from("<BBH", data, p)
        assert zero == 0 and leaf in (0, 1) and count <= bs
        body = data[p + 4:p + 4 + bs * item_bytes]
        assert len(body) == bs * item_bytes and not any(body[count * item_bytes:]), "node padding"
        out.append((leaf, [body[i * item_bytes:(i + 1) * item_bytes] for i in range(count)]))
    return out


def chrom_tree(data, at, option_bs=None):
    """-> ({block_size, key_size, n}, [(name bytes, chromId, chromSize)] in key order, the offset behind the tree)"""
    magic, bs, ks, vs, n, zero = struct.unpack_from("<IIIIQQ", data, at)
    assert magic == CHROM_MAGIC and vs == 8 and zero == 0 and bs >= 1
    if option_bs is not None:
        assert bs == min(option_bs, max(n, 1))
    _, items = levels_of(n, bs)
    item = ks + 8
    p = at + 32
    starts = {}
    for l in range(len(items) - 1, -1, -1):   # the root's level first
        starts[l] = p
        p += max(-(-items[l] // bs), 1) * (4 + bs * item)
    first_keys, out = {}, []
    for l in range(len(items)):
        nodes = _nodes(data, starts[l], bs, item, max(-(-items[l] // bs), 1))
        assert sum(len(it) for _, it in nodes) == items[l] and all(len(it) == bs for _, it in nodes[:-1]), "a level is filled left to right"
        keys = []
        for k, (leaf, its) in enumerate(nodes):
            assert leaf == (1 if l == 0 else 0)
            for i, b in enumerate(its):
                key = b[:ks]
                keys.append(key)
                if l == 0:
                    cid, size = struct.unpack("<II", b[ks:])
                    name = key.rstrip(b"\0")
                    assert name and key == name + b"\0" * (ks - len(name))
                    out.append((name, cid, size))
                else:
                    child, = struct.unpack("<Q", b[ks:])
                    idx = k * bs + i
                    assert child == starts[l - 1] + idx * (4 + bs * item), "child offset"
                    assert key == first_keys[l - 1][idx * bs], "an inner key is the first key below"
        assert keys == sorted(keys) and len(set(keys)) == len(keys), "key order"
        first_keys[l] = keys
    assert [c for _, c, _ in out] == list(range(n)) and (not out or max(len(nm) for nm, _, _ in out) == ks)
    return {"block_size": bs, "key_size": ks, "n": n}, out, p


def _bounds(b):
    sc, sb, ec, eb = struct.unpack("<IIII", b[:16])
    return (sc, sb), (ec, eb)


def rtree(data, at, option_bs=None):
    """-> ({block_size, n, lo, hi, end}, the leaf items [(lo, hi, offset, size)], the offset behind the tree).  lo / hi are (chrom, base)"""
    magic, bs, n, sc, sb, ec, eb, end, per_slot, zero = struct.unpack_from("<IIQIIIIQII", data, at)
    assert magic == RTREE_MAGIC and per_slot == 1 and zero == 0 and bs >= 1
    if option_bs is not None:
        assert bs == min(option_bs, max(n, 1))
    _, items = levels_of(n, bs)
    p = at + 48
    starts = {}
    for l in range(len(items) - 1, -1, -1):
        starts[l] = p
        p += max(-(-items[l] // bs), 1) * (4 + bs * (32 if l == 0 else 24))
    below, leaves = None, []
    for l in range(len(items)):
        size = 32 if l == 0 else 24
        nodes = _nodes(data, starts[l], bs, size, max(-(-items[l] // bs), 1))
        assert sum(len(it) for _, it in nodes) == items[l] and all(len(it) == bs for _, it in nodes[:-1])
        level = []
        for k, (leaf, its) in enumerate(nodes):
            assert leaf == (1 if l == 0 else 0)
            for i, b in enumerate(its):
                lo, hi = _bounds(b)
                assert lo < hi
                idx = k * bs + i
                if l == 0:
                    off, sz = struct.unpack("<QQ", b[16:])
                    leaves.append((lo, hi, off, sz))
                else:
                    child, = struct.unpack("<Q", b[16:])
                    assert child == starts[l - 1] + idx * (4 + bs * (32 if l == 1 else 24)), "child offset"
                    kids = below[idx * bs:(idx + 1) * bs]
                    assert lo == min(c[0] for c in kids) and hi == max(c[1] for c in kids), "an inner item bounds its children exactly"
                level.append((lo, hi))
        assert [b[0] for b in level] == sorted(b[0] for b in level), "items are ordered by (chrom, start)"
        below = level
    if n:
        assert (sc, sb) == min(b[0] for b in below) and (ec, eb) == max(b[1] for b in below), "the header bounds the root"
    else:
        assert (sc, sb, ec, eb) == (0, 0, 0, 0)
    return {"block_size": bs, "n": n, "lo": (sc, sb), "hi": (ec, eb), "end": end}, leaves, p


def query(data, at, chrom, start, end):
    """the leaf items [(offset, size)] whose bounds overlap [start, end) of chrom, found by descending from the root"""
    magic, bs, n = struct.unpack_from("<IIQ", data, at)
    _, items = levels_of(n, bs)
    lo_q, hi_q = (chrom, start), (chrom, end)
    out = []

    def descend(p):
        leaf, _, count = struct.unpack_from("<BBH", data, p)
        size = 32 if leaf else 24
        for i in range(count):
            b = data[p + 4 + i * size:p + 4 + (i + 1) * size]
            lo, hi = _bounds(b)
            if lo < hi_q and hi > lo_q:
                if leaf:
                    out.append(struct.unpack("<QQ", b[16:]))
                else:
                    descend(struct.unpack("<Q", b[16:])[0])
    descend(at + 48)
    return out


def payload(data, off, size, compressed):
    raw = bytes(data[off:off + size])
    return zlib.decompress(raw) if compressed else raw


def section(raw):
    """-> (chromId, chromStart, chromEnd, items) of one decoded section"""
    cid, cs, ce, step, span, typ, zero, count = struct.unpack_from("<IIIIIBBH", raw, 0)
    assert (step, span, typ, zero) == (0, 0, 1, 0) and len(raw) == 24 + 12 * count and count >= 1
    items = np.frombuffer(raw, dtype=ITEM, offset=24)
    assert cs == items["start"][0] and ce == items["end"][-1] and np.all(items["start"] < items["end"]) and np.all(items["end"][:-1] <= items["start"][1:])
    return cid, cs, ce, items


def read_all(data, option_bs=None, items_per_slot=None):
    """The whole file, walked and checked: -> dict of header, chroms, tree headers, sections [(chromId, start, end, items)], and per
    zoom level its reduction, tree header and records.  What lies between the parts is checked to be nothing: every part begins
    where the one before it ends."""
    h = header(data)
    compressed = h["uncompress_buf"] != 0
    ct, chroms, p = chrom_tree(data, h["chrom_tree"], option_bs)
    assert p == h["full_data"]

    def part(data_off, index_off, count_fmt):
        count, = struct.unpack_from(count_fmt, data, data_off)
        th, leaves, behind = rtree(data, index_off, option_bs)
        q = data_off + struct.calcsize(count_fmt)
        for lo, hi, off, size in leaves:
            assert off == q and size > 0, "the items lie back to back"
            q += size
        assert q == index_off == th["end"]
        return count, th, leaves, behind
    n_sec, th, leaves, p = part(h["full_data"], h["full_index"], "<Q")
    assert n_sec == th["n"] == len(leaves)
    sections = []
    for lo, hi, off, size in leaves:
        raw = payload(data, off, size, compressed)
        assert not compressed or len(raw) <= h["uncompress_buf"]
        cid, cs, ce, items = section(raw)
        assert lo == (cid, cs) and hi == (cid, ce) and (items_per_slot is None or len(items) <= items_per_slot)
        sections.append((cid, cs, ce, items))
    assert [(s[0], s[1]) for s in sections] == sorted((s[0], s[1]) for s in sections)
    out = {"header": h, "chrom_tree": ct, "chroms": chroms, "full_index": th, "sections": sections, "zooms": [], "compressed": compressed}
    for z in h["zooms"]:
        assert z["data"] == p
        n_rec, zt, zl, p = part(z["data"], z["index"], "<I")
        blocks = []
        for lo, hi, off, size in zl:
            raw = payload(data, off, size, compressed)
            assert len(raw) % 32 == 0 and (not compressed or len(raw) <= h["uncompress_buf"])
            rec = np.frombuffer(raw, dtype=ZOOM)
            assert lo == (int(rec["chrom"][0]), int(rec["start"][0])) and hi == (int(rec["chrom"][-1]), int(rec["end"][-1]))
            assert items_per_slot is None or len(rec) <= items_per_slot
            blocks.append(rec)
        rec = np.concatenate(blocks) if blocks else np.zeros(0, dtype=ZOOM)
        assert len(rec) == n_rec and np.all(rec["valid"] > 0) and np.all(rec["end"] - rec["start"] <= z["reduction"]) and np.all(rec["start"] % z["reduction"] == 0)
        out["zooms"].append({"reduction": z["reduction"], "index": zt, "records": rec, "block_sizes": [len(b) for b in blocks]})
    assert p + 4 == len(data)
    return out


def intervals(data, chrom_id, start, end):
    """the items (start, end, value) of the full data that overlap [start, end) of a chromosome, through the R-tree"""
    h = header(data)
    got = []
    for off, size in query(data, h["full_index"], chrom_id, start, end):
        cid, _, _, items = section(payload(data, off, size, h["uncompress_buf"] != 0))
        if cid == chrom_id:
            got += [(int(i["start"]), int(i["end"]), float(i["value"])) for i in items if i["start"] < end and i["end"] > start]
    return got

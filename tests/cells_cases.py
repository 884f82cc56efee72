"""The definitions of br_cells and of br_dedup's "cell_source" (include/bramble_amd.h) restated in plain Python float64, entry by entry in
the stated orders, and the inputs of their tests.

The restatement works from what a run leaves: per read name the list of its records (bytes from refID on, without block_size; the
inputs' builders are tests/dedup_cases.py's) -- the barcode from the first record, the class from the records' refIDs (the transcript
ids of projected records).  `order` re-orders every sum of the EM ("forward": as defined; "reversed"; an int: a seeded shuffle): what
the order of a sum alone does to a result is the yardstick of the GPU tests' accuracy rule."""
import numpy as np

from tests import bamio
from tests import dedup_cases as dc

SOURCES = {"name": 0, "tag": 1}
MODES = {"unique": 0, "uniform": 1, "em": 2}
BC_MAX = 32
NONE = 0xffffffff


# ---- the restatement -------------------------------------------------------------------------------------------------------------
def barcode_of_record(rec, source="name", sep=b"_", tag=b"CB"):
    """-> (barcode bytes or None, why): why in ("", "none", "too_long", "bad_aux")"""
    f = bamio.record_fields(rec)
    bc = None
    if source == "name":
        p2 = f["name"].rfind(sep)
        p1 = f["name"].rfind(sep, 0, p2) if p2 >= 0 else -1
        if p1 >= 0:
            bc = f["name"][p1 + 1:p2]
    else:
        fields, clean = dc.aux_walk(f["aux"])
        for t, typ, val in fields:
            if t == tag and typ == ord("Z"):
                bc = val[:-1]
                break
        if bc is None and not clean:
            return None, "bad_aux"
    if bc is None or len(bc) == 0:
        return None, "none"
    if len(bc) > BC_MAX:
        return None, "too_long"
    return bytes(bc), ""


def barcodes_of(groups, source="name", sep=b"_", tag=b"CB"):
    """-> (per name its barcode or None, {"no_barcode", "too_long", "bad_aux"}); a name without records has none and is counted nowhere"""
    out, cnt = [], {"no_barcode": 0, "too_long": 0, "bad_aux": 0}
    for g in groups:
        if not g:
            out.append(None)
            continue
        b, why = barcode_of_record(g[0], source, sep, tag)
        out.append(b)
        cnt["no_barcode"] += b is None
        cnt["too_long"] += why == "too_long"
        cnt["bad_aux"] += why == "bad_aux"
    return out, cnt


def classes_of(groups, dropped=None):
    """-> (name_cls uint32 per name, NONE for a name without records or a dropped one; the classes as ascending tuples of transcript
    ids, numbered by their first name)"""
    index, classes, out = {}, [], []
    for i, g in enumerate(groups):
        if not g or (dropped is not None and dropped[i]):
            out.append(NONE)
            continue
        labels = tuple(sorted({bamio.record_fields(r)["ref_id"] for r in g}))
        if labels not in index:
            index[labels] = len(classes)
            classes.append(labels)
        out.append(index[labels])
    return np.asarray(out, dtype=np.uint32), classes


def bc_key(b):
    return (len(b), b)


def model_of(barcodes, name_cls, classes, tx_feature):
    """-> {"cells": the barcodes in (length, bytes) order, "name_cell": uint32 per name, "entries": per cell [(class, n_e, F_e)] in
    ascending class order, "slots": per cell the ascending distinct features}"""
    counted = [i for i, b in enumerate(barcodes) if b is not None and name_cls[i] != NONE]
    cells = sorted({barcodes[i] for i in counted}, key=bc_key)
    at = {b: k for k, b in enumerate(cells)}
    name_cell = np.full(len(barcodes), NONE, dtype=np.uint32)
    per = [dict() for _ in cells]
    for i in counted:
        k = at[barcodes[i]]
        name_cell[i] = k
        per[k][int(name_cls[i])] = per[k].get(int(name_cls[i]), 0) + 1
    entries, slots = [], []
    for mine in per:
        es = [(c, mine[c], tuple(sorted({int(tx_feature[t]) for t in classes[c]}))) for c in sorted(mine)]
        entries.append(es)
        slots.append(sorted({f for _, _, fs in es for f in fs}))
    return {"cells": cells, "name_cell": name_cell, "entries": entries, "slots": slots}


def _ordered(items, order, rng):
    items = list(items)
    if order == "reversed":
        return items[::-1]
    if order != "forward":
        return [items[i] for i in rng.permutation(len(items))]
    return items


def _sum(values):
    s = 0.0
    for v in values:
        s += v
    return s


def em_cell(entries, slots, max_iters, tolerance, order="forward"):
    """-> (theta per slot, iterations run)"""
    rng = np.random.default_rng(order if isinstance(order, int) else 0)
    at = {f: s for s, f in enumerate(slots)}
    of_entry = [_ordered([at[f] for f in fs], order, rng) for _, _, fs in entries]
    into = [[] for _ in slots]
    for e, (_, _, fs) in enumerate(entries):
        for f in fs:
            into[at[f]].append(e)
    into = [_ordered(x, order, rng) for x in into]
    theta, it = [1.0] * len(slots), 0
    while it < max_iters:
        q = []
        for e, (_, n_e, _) in enumerate(entries):
            d = _sum(theta[s] for s in of_entry[e])
            q.append(n_e / d if d != 0 else 0.0)
        new = [theta[s] * _sum(q[e] for e in into[s]) for s in range(len(slots))]
        rel = max([abs(n - t) / n for n, t in zip(new, theta) if n > 1e-8] + [0.0])
        theta, it = new, it + 1
        if rel < tolerance:
            break
    return theta, it


def unique_cell(entries, slots):
    val = {f: 0 for f in slots}
    for _, n_e, fs in entries:
        if len(fs) == 1:
            val[fs[0]] += n_e
    return [float(val[f]) for f in slots]


def matrix_of(model, mode, max_iters=10000, tolerance=1e-2, order="forward"):
    """-> {"off", "feature", "value": CSR by cell; "names", "unique", "multi", "features", "iterations": per cell}"""
    off, feat, val = [0], [], []
    st = {k: [] for k in ("names", "unique", "multi", "features", "iterations")}
    for es, slots in zip(model["entries"], model["slots"]):
        if mode == "unique":
            v, it = unique_cell(es, slots), 0
            keep = [x != 0 for x in v]
        else:
            v, it = em_cell(es, slots, 1 if mode == "uniform" else max_iters, 0.0 if mode == "uniform" else tolerance, order)
            keep = [True] * len(v)
        feat += [f for f, k in zip(slots, keep) if k]
        val += [x for x, k in zip(v, keep) if k]
        off.append(len(feat))
        uniq = sum(n for _, n, fs in es if len(fs) == 1)
        multi = sum(n for _, n, fs in es if len(fs) != 1)
        for k, x in zip(("names", "unique", "multi", "features", "iterations"), (uniq + multi, uniq, multi, sum(keep), it)):
            st[k].append(x)
    out = {"off": np.asarray(off, np.uint64), "feature": np.asarray(feat, np.uint32), "value": np.asarray(val, np.float64)}
    out.update({k: np.asarray(v, np.uint64 if k in ("names", "unique", "multi") else np.uint32) for k, v in st.items()})
    return out


def spread_of(model, mode, max_iters):
    """(the forward matrix at tolerance 0, s): s = the largest relative difference, over values > 1e-6, between the restatement's
    forward, reversed and seeded-shuffle summation orders"""
    runs = [matrix_of(model, mode, max_iters, 0.0, o) for o in ("forward", "reversed", 12345)]
    ref = runs[0]["value"]
    m = ref > 1e-6
    s = max(float(np.max(np.abs(r["value"][m] - ref[m]) / ref[m])) for r in runs[1:])
    return runs[0], s


def per_cell_molecules(method, groups, umis, barcodes):
    """br_dedup with "cell_source": rep per name over the (signature, barcode) position groups"""
    keys = [None if s is None else (s, b or b"") for s, b in zip(dc.signatures_of(groups), barcodes)]
    return dc.molecules_of(method, keys, umis), dc.groups_of(keys)


def barcode_matrix(barcodes):
    return dc.umi_matrix(barcodes)


# ---- the inputs --------------------------------------------------------------------------------------------------------------------
N_TX, N_FEATURES = 160, 80
TX_FEATURE = np.arange(N_TX, dtype=np.uint32) // 2
ACGT = np.frombuffer(b"ACGT", np.uint8)
LDS_LOW = 1400   # an "lds_bytes" at which a mid-sized cell of standard_run stays in LDS and another takes the HBM route


def _bc(rng, n=12):
    return bytes(rng.choice(ACGT, size=n).tolist())


def _name(k, bc, tids, umi=b"ACGTAC", pos=100, aux=b""):
    """a read name READ_CB_UMI with one row per transcript of `tids`"""
    nm = b"r%d" % k + (b"_" + bc if bc is not None else b"") + (b"_" + umi if umi is not None else b"")
    return dc.name_row(nm, [(int(t), pos + 3 * j, dc.cig("30M"), 0) for j, t in enumerate(tids)], aux)


def standard_run(seed=0):
    """About 70 cells over N_TX transcripts and N_FEATURES features (transcripts 2g and 2g + 1 are feature g): 40 cells of one entry;
    cells of 64 and of 65 slots; one of 65 pairs on 48 slots; one whose feature 0 sits in 71 entries; one with an entry of 66
    features; about 25 cells of 4 to 120 names over a pool of classes; and the names that count nowhere: without a barcode, with one
    separator, with a barcode of 33 bytes (one of 32 counts), without rows.  The names of the cells are interleaved."""
    rng = np.random.default_rng(seed)
    names = []   # (barcode, tids)
    for k in range(40):   # one entry each
        bc = _bc(rng)
        tids = [[k], [2 * k, 2 * k + 1], [k, k + 40]][k % 3]
        names += [(bc, tids)] * (1 + k % 3)
    a, b, c, d, e = (_bc(rng, 10 + i) for i in range(5))
    names += [(a, [2 * g]) for g in range(64)]                                   # 64 slots, 64 pairs: a wave's
    names += [(b, [2 * g + 1]) for g in range(65)] + [(b, [3]), (b, [0, 2])]     # 65 slots: a block's
    names += [(c, [2 * g]) for g in range(48)] + [(c, [2 * g, 2 * g + 2]) for g in range(8)] + [(c, [5])]   # 48 + 16 + 1 pairs, 48 slots
    names += [(d, [0, 2 * g]) for g in range(1, 71)] + [(d, [0])] * 3 + [(d, [1, 9])]   # feature 0 in 72 entries
    names += [(e, [2 * g for g in range(66)])] * 2 + [(e, [2 * g]) for g in range(0, 66, 5)] + [(e, [4, 6, 8])]
    pool = [[int(t)] for t in rng.integers(0, N_TX, 12)] + [sorted(set(int(t) for t in rng.integers(0, 60, 2))) for _ in range(10)] + \
           [sorted(set(int(t) for t in rng.integers(0, 30, 3))) for _ in range(8)]
    for k in range(25):
        bc = _bc(rng, 8 + k % 9)
        n = int(rng.integers(4, 30)) if k % 6 else 120
        names += [(bc, pool[int(rng.integers(len(pool)))]) for _ in range(n)]
    long32 = _bc(rng, 32)
    names += [(long32, [7]), (long32, [7, 9]), (_bc(rng, 33), [7]), (None, [11])]
    order = rng.permutation(len(names))
    run = [_name(i, names[j][0], names[j][1], umi=_bc(rng, 6)) for i, j in enumerate(order)]
    run.insert(5, dc.name_row(b"onesep_ACGTACGT", [(3, 50, dc.cig("30M"), 0)]))
    run.insert(9, dc.name_row(b"plain", [(3, 50, dc.cig("30M"), 16)]))
    run.insert(13, dc.name_row(b"norows_" + a + b"_ACGTAC", []))
    run.insert(17, dc.name_row(b"empty__ACGTAC", [(3, 50, dc.cig("30M"), 0)]))
    return run


def tagged(run, tag=b"CB"):
    """the same names carrying their name's barcode in CB:Z behind an NH field; one name's aux is cut inside a field in front of it"""
    out = []
    for i, nm in enumerate(run):
        parts = nm["name"].split(b"_")
        bc = parts[-2] if len(parts) >= 3 else b""
        aux = b"NHC\x01" + (tag + b"Z" + bc + b"\0" if bc else b"")
        if i == 21:
            aux = b"XSi\x01\x02"   # a field that runs past the record's end
        out.append(dc.name_row(nm["name"], nm["rows"], aux))
    return out


def dropped_flags(n, seed=3):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 10, n) == 0).astype(np.uint8)


def stopping_run(seed=5):
    """cells whose EM stops early at the default tolerance, after different numbers of iterations"""
    rng = np.random.default_rng(seed)
    names = []
    for k in range(70):
        bc = _bc(rng, 10)
        g = int(rng.integers(0, 30))
        n_a, n_b, n_ab = int(rng.integers(1, 40)), int(rng.integers(1, 40)), int(rng.integers(1, 60))
        names += [(bc, [2 * g])] * n_a + [(bc, [2 * g + 2])] * n_b + [(bc, [2 * g, 2 * g + 2])] * n_ab
        if k % 4 == 0:
            names += [(bc, [2 * g, 2 * g + 2, 2 * g + 4])] * int(rng.integers(1, 20)) + [(bc, [2 * g + 4])] * (k % 3)
    order = rng.permutation(len(names))
    return [_name(i, names[j][0], names[j][1]) for i, j in enumerate(order)]


def dedup_run(seed=7):
    """br_dedup per cell: the same UMI and signature in two cells (two molecules) and again inside one cell (one molecule); one-mismatch
    UMIs inside a cell and across cells; names without a barcode; around it the standard cells' names with few distinct UMIs, so
    that cells share signatures and UMIs all over"""
    rng = np.random.default_rng(seed)
    sig = [(3, 500, dc.cig("30M"), 0)]
    run = [dc.name_row(b"m0_AAAACCCC_ACGTAC", sig), dc.name_row(b"m1_GGGGTTTT_ACGTAC", sig), dc.name_row(b"m2_AAAACCCC_ACGTAC", sig),
           dc.name_row(b"m3_AAAACCCC_ACGTAA", sig), dc.name_row(b"m4_GGGGTTTT_ACGTAA", sig), dc.name_row(b"m5_GGGGTTTT_ACGTAA", sig),
           dc.name_row(b"m6_GGGGTTTT_ACGTAA", sig), dc.name_row(b"m7_ACGTAC", sig), dc.name_row(b"m8_ACGTAC", sig), dc.name_row(b"m9__ACGTAC", sig)]
    umis = [_bc(rng, 6) for _ in range(3)]
    umis.append(dc.mutate(umis[0], 2))
    base = standard_run(seed)
    for i, nm in enumerate(base):
        parts = nm["name"].split(b"_")
        if len(parts) >= 3:
            parts[-1] = umis[int(rng.integers(len(umis)))]
        rows = [(t, 100, ops, fl) for t, _, ops, fl in nm["rows"]][:3]   # few positions: the cells share signatures
        run.append(dc.name_row(b"_".join(parts), rows, nm["aux"]))
    return run


# ---- record streams in: the command line's inputs ------------------------------------------------------------------------------------
def with_cells_records(recs, n_cells=12, seed=0):
    """every read-name group of `recs` (framed records, collated) re-emitted under <orig>.<j>_<CB>_<UMI>: one to three copies with the
    group's UMI, the third in the next cell (the same UMI and placements in two cells are two molecules), every seventh group without
    a barcode (<orig>.<j>_<UMI>) and every eleventh with a second UMI one mismatch away -> the framed records"""
    rng = np.random.default_rng(seed)
    cells = [_bc(rng, 8 + k % 3) for k in range(n_cells)]
    groups = []
    for r in recs:
        nm = bytes(r[36:36 + r[12] - 1])
        if groups and groups[-1][0] == nm:
            groups[-1][1].append(r)
        else:
            groups.append((nm, [r]))
    out = []
    for i, (nm, mine) in enumerate(groups):
        k = int(rng.integers(n_cells))
        u = dc.random_umi(rng)
        for j in range(1 + i % 3):
            cb = cells[(k + (j == 2)) % n_cells]
            umi = dc.mutate(u, 3) if i % 11 == 0 and j == 1 else u
            name = nm.replace(b"_", b"-") + b".%d" % j + (b"_" + cb if i % 7 else b"") + b"_" + umi
            out += [dc.renamed(bytes(r), name) for r in mine]
    return out

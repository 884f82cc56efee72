#!/usr/bin/env python3
"""Secondary configurations of BASELINE.json (not the bench contract line; numbers for BASELINE.md):

  python bench_extra.py c5 [--reads N]   HiFi-like --lr-hq --strict --similarity-threshold 0.95 (configs[4], 1 GPU)
  python bench_extra.py c3 [--reads N]   ONT-like --lr -S with a synthetic genome: clip rescue incl. k_ksw GCUPS (configs[2])
  python bench_extra.py bam [--reads N]  re-encode the rows of configs[1] as BAM records (device part)
  python bench_extra.py bundle [--reads N]  raw BAM records resident in HBM -> projected BAM records (br_project_bam_device)
  python bench_extra.py cli [--reads N] [--threads T]  the command line file to file (BGZF inflate, device path, BGZF deflate)
  python bench_extra.py sam [--reads N]  SAM text input: device parse time per chunk (hipEvents), text GB/s and records/s of
                                         br_sam_reader, and the command line file to file for the workload of `cli` as SAM and as BAM
  python bench_extra.py collate [--reads N]  br_collator over N pairs' records (default 10 M pairs, ~20 M records) in HBM in a
                                         random order, added in bundles of 1 M: add / finish / bundle-cut seconds, collator
                                         peak device bytes per record, against br_bam_split_device over the same stream
  python bench_extra.py sort [--reads N]  br_sorter over the projected records of the bench.py workload (N pairs, default 10 M): handed
                                         to the sorter from HBM in slices of 1 M rows, finished, then drained with next (128 MiB
                                         pieces) into br_bgzf_deflate_device: add / finish / drain seconds (the gather's share of the
                                         drain apart), sorter peak device bytes per record
  python bench_extra.py quant [--reads N]  br_quant over the rows of the bench.py workload (N pairs, default 10 M), projected once
                                         (br_project_batch_device, timed): the read names handed over from HBM in slices of 1 M
                                         alignments, the classes, the EM -- seconds in add / finish / em, iterations, names, classes,
                                         labels, quantifier peak device bytes per read name; then the same with the fragment-length
                                         model ("eff_len": the adds through br_quant_add_rows), as runs_eff_length
  python bench_extra.py quant_genes [--reads N] [--bootstraps B]   the gene level on the quant workload: br_quant_genes' seconds beside
                                         br_quant_finish's of the same run, br_quant_gene_result, and br_quant_gene_boot_summary
                                         (the first call, which makes the B x G table, and a second) beside br_quant_boot_summary
  python bench_extra.py quant_boot [--reads N] [--bootstraps B] [--boot-chunk W]  the bootstrap replicates on the quant workload, in one
                                         process: br_quant_em (seconds, iterations, seconds per replicate-iteration), then
                                         br_quant_bootstrap with B replicates (default 32; W of them together, 0: the library's
                                         default), sampling and EM seconds apart (br_quant_boot_stats), seconds per
                                         replicate-iteration and the ratio of the two
  python bench_extra.py coverage [--reads N]  br_coverage over the rows of the bench.py workload (N pairs, default 10 M), projected once
                                         (br_project_batch_device, timed) and resident in HBM: all rows in one add, then finish --
                                         br_coverage_stats' add and finish seconds, rows, bases, runs, peak device bytes per base; the
                                         same in slices of 1 M rows; and, for comparison, br_quant_add_rows with "eff_len" on over the
                                         same rows in the same process (the same shape of pass over a, cigar and pool)
  python bench_extra.py samout [--reads N]  SAM text out: br_sam_format_device on the projected records of N pairs (default 500 000,
                                         about 1 M records: one CLI bundle) against br_bgzf_deflate_device of the same stream in the
                                         same process (ms per bundle, text GB/s), then the command line file to file with -O sam
                                         against the default BAM, alternated (SAMOUT_CLI_RUNS pairs, default 3; 0 skips them)
  python bench_extra.py cells [--reads K]  br_cells on seeded synthetic tables fed straight to br_quant + br_cells from HBM: K cells (default
                                         10 000) of 300 read names over 200 of the cell's transcripts each (one to three a name, two
                                         transcripts a gene), plus a tail of 5 K barcodes of one to five names; mode em at the default
                                         tolerance.  add / finish seconds and the value kernel's seconds: all cells at the default
                                         "lds_bytes" (one launch, wave and block routes), the same with "lds_bytes" 0 (the block cells on
                                         scratch in HBM), the large cells alone (block route), the tail alone (wave route)
  python bench_extra.py whitelist [--reads N]  br_whitelist of 6 794 880 random 16-mers (the size of the 10x v3 list) and N read names
                                         (default 4 M, one row each) over 100 000 of them, 1 % with one substituted base, fed to
                                         br_quant + br_cells from HBM: build seconds and the longest probe chain, then per step
                                         br_cells_finish (mode unique) without a whitelist and with it under 1mm and 1mm-multi -- the
                                         resolve's seconds, the statuses' names and, beside them, the finish's seconds without the resolve
  python bench_extra.py cellcall [--reads K]  br_cellcall at its default parameters (emptydrops, 10 000 simulations) on a seeded generated
                                         CSR resident in HBM: K barcodes (default 300 000) x 30 000 features, 4 000 large cells, 6 000
                                         barcodes of 500 .. 2 000 counts (half from the cells' profile, half ambient) and an ambient
                                         tail: the four stage times of br_cellcall_stats (rank, ambient, simulate, p-value), the whole
                                         run, the calls; and, for scale, the tests' restatement over 100 of the simulations on the CPU
  python bench_extra.py small            small calls: us per device-resident step at 1 .. 52 000 pairs (without the per-kernel
                                         events bench.py keeps on), the path without host round trips against the ordinary one,
                                         and br_project_group / br_project_groups host to host from plain C (profiles/group_latency.c)

Same protocol as bench.py: inputs resident in HBM, warmup, hipEvent kernel times, one JSON line.
"""
import argparse
import json
import os

import numpy as np
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", choices=["c3", "c5", "bam", "bundle", "cli", "small", "inflate", "sam", "collate", "samout", "sort", "quant", "quant_boot", "quant_genes", "coverage", "cells", "whitelist", "cellcall"])
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reads", type=int, default=0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--bootstraps", type=int, default=32)
    ap.add_argument("--boot-chunk", type=int, default=0)
    args = ap.parse_args()
    import torch
    from bramble_amd import device as brdev
    from bramble_amd import lib, synth
    if args.config == "cellcall":
        K, F, n_large, n_mid = args.reads or 300_000, 30_000, 4_000, 6_000
        rng = np.random.default_rng(13)
        amb = rng.gamma(0.3, 1.0, F) + 1e-4
        amb /= amb.sum()
        cellp = rng.permutation(amb) * rng.gamma(2.0, 1.0, F)
        cellp /= cellp.sum()
        totals = np.concatenate([rng.integers(5000, 20001, n_large), rng.integers(500, 2001, n_mid), np.minimum(rng.geometric(0.03, K - n_large - n_mid), 450)])
        like_cell = np.concatenate([np.ones(n_large, bool), rng.random(n_mid) < 0.5, np.zeros(K - n_large - n_mid, bool)])
        perm = rng.permutation(K)   # (the barcodes in no order of size)

        def draws(mask, prof):
            cells = np.repeat(perm[np.flatnonzero(mask)], totals[mask]).astype(np.int64)
            return cells * F + rng.choice(F, len(cells), p=prof)
        key, cnt = np.unique(np.concatenate([draws(like_cell, cellp), draws(~like_cell, amb)]), return_counts=True)
        off = np.searchsorted(key // F, np.arange(K + 1)).astype(np.uint64)
        feat = (key % F).astype(np.uint32)
        t = [torch.from_numpy(x).cuda() for x in (off.view(np.int64), feat.view(np.int32), cnt.astype(np.uint32).view(np.int32))]
        torch.cuda.synchronize()
        out = {"config": "cellcall", "workload": "%d barcodes x %d features, %d entries, %d counts; %d large cells, %d of 500..2000 counts (%d of them cell-like)"
               % (K, F, len(key), int(cnt.sum()), n_large, n_mid, int(like_cell[n_large:].sum())), "runs": []}
        c = None
        for step in range(args.warmup + args.steps):
            if c is not None:
                c.close()
            c = lib.CellCall(keep_sims=0)
            t0 = time.perf_counter()
            c.run_device(t[0], t[1], t[2], F)
            wall = time.perf_counter() - t0
            st = c.stats()
            if step >= args.warmup:
                run = {k[:-3] + "_s": round(st[k] * 1e-6, 4) for k in ("rank_us", "ambient_us", "simulate_us", "pvalue_us")}
                run.update({"run_s": round(wall, 4)})
                run.update({k: st[k] for k in ("called_simple", "called_emptydrops", "threshold", "candidates", "n_max", "wanted_totals", "active_features",
                                               "p_route", "sim_chunks", "fallback", "sims", "peak_bytes")})
                out["runs"].append(run)
        status = c.calls()[0]
        mid = perm[n_large:n_large + n_mid]
        out["mid_cell_like_called"] = int(np.sum(status[mid[like_cell[n_large:n_large + n_mid]]] == 2))
        out["mid_ambient_called"] = int(np.sum(status[mid[~like_cell[n_large:n_large + n_mid]]] == 2))
        try:   # for scale only: the tests' restatement (numpy, one thread) over 100 of the simulations, on this host's CPU
            from tests import cellcall_cases
            a, ln, want = c.ambient(), c.logtable(), c.wanted()
            t0 = time.perf_counter()
            cellcall_cases.simulate(a["T"], a["lp"], ln, st["n_max"], 100, 0, [int(x) for x in want])
            out["restatement_100_sims_s"] = round(time.perf_counter() - t0, 3)
        except ImportError:
            pass
        c.close()
        print(json.dumps(out))
        return
    if args.config == "whitelist":
        n_wl, n_names, n_cells, n_tx = 6_794_880, args.reads or 4_000_000, 100_000, 20_000
        rng = np.random.default_rng(7)
        acgt = np.frombuffer(b"ACGT", np.uint8)
        wl = np.zeros((n_wl, 32), np.uint8)
        wl[:, :16] = rng.choice(acgt, size=(n_wl, 16))
        ln = np.full(n_wl, 16, np.uint8)
        cells = rng.choice(n_wl, n_cells, replace=False)
        bc = wl[cells[rng.integers(0, n_cells, n_names)], :16].copy()
        bad = np.flatnonzero(rng.random(n_names) < 0.01)
        pos = rng.integers(0, 16, len(bad))
        bc[bad, pos] = acgt[(np.searchsorted(acgt, bc[bad, pos]) + rng.integers(1, 4, len(bad))) % 4]   # another base
        # one row a name; [block_size][32 fixed bytes][r_<16>_<UMI> NUL]
        l_name = 2 + 16 + 1 + 8 + 1
        rec = np.zeros((n_names, 36 + l_name), np.uint8)
        rec[:, 0] = 32 + l_name
        rec[:, 12] = l_name
        rec[:, 36], rec[:, 37], rec[:, 54] = ord("r"), ord("_"), ord("_")
        rec[:, 38:54] = bc
        rec[:, 55:63] = np.frombuffer(b"ACGTACGT", np.uint8)
        a = np.zeros((n_names, 4), np.uint32)
        a[:, 0] = rng.integers(0, n_tx, n_names)
        row_off = np.arange(n_names + 1, dtype=np.uint64)
        group_off = np.arange(n_names + 1, dtype=np.uint32)
        rec_off = np.arange(n_names + 1, dtype=np.uint64) * np.uint64(rec.shape[1])
        t = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), row_off.view(np.int64), group_off.view(np.int32), rec.reshape(-1), rec_off.view(np.int64))]
        recs = lib.BrDeviceBam(t[3].data_ptr(), t[3].numel(), t[4].data_ptr(), t[4].numel() - 1)
        tx_feature = np.arange(n_tx, dtype=np.uint32) // 2
        torch.cuda.synchronize()
        out = {"config": "whitelist", "workload": "%d random 16-mers, %d read names over %d of them, %d with one substituted base" % (n_wl, n_names, n_cells, len(bad)),
               "builds": [], "runs": []}
        w = None
        for step in range(args.warmup + args.steps):
            if w is not None:
                w.close()
            w = lib.Whitelist((wl, ln))
            st = w.stats()
            if step >= args.warmup:
                out["builds"].append({"build_s": round(st["build_us"] * 1e-6, 3), "distinct": st["distinct"], "slots": st["slots"], "longest_chain": st["longest_chain"],
                                      "held_bytes": st["held_bytes"], "peak_bytes": st["peak_bytes"]})
        for step in range(args.warmup + args.steps):
            for correct in (None, "1mm", "1mm-multi"):
                q = lib.Quant(n_tx)
                q.set_param("keep_names", 1)
                c = lib.Cells(mode=0)
                if correct:
                    c.set_whitelist(w, correct)
                for g0 in range(0, n_names, 1_000_000):
                    g1 = min(n_names, g0 + 1_000_000)
                    q.add_device(t[0], t[1], t[2], g0, g1)
                    c.add_device(t[1], t[2], recs, g0, g1)
                q.finish()
                n_c, _ = c.finish(q, tx_feature, n_tx // 2)
                st = c.stats()
                run = {"correct": correct, "cells": n_c, "finish_s": round(st["finish_us"] * 1e-6, 4)}
                if correct:
                    ws = c.whitelist_stats()
                    run.update({"resolve_s": round(ws["resolve_us"] * 1e-6, 4), "finish_without_resolve_s": round((st["finish_us"] - ws["resolve_us"]) * 1e-6, 4)})
                    run.update({k: ws[k] for k in ("exact", "corrected", "no_match", "ambiguous", "distinct_observed")})
                c.close()
                q.close()
                if step >= args.warmup:
                    out["runs"].append(run)
        w.close()
        print(json.dumps(out))
        return
    if args.config == "cells":
        k_cells = args.reads or 10_000
        n_tx, per_cell, own = 20_000, 300, 200
        rng = np.random.default_rng(11)

        def barcodes(n, width):
            return rng.choice(np.frombuffer(b"ACGT", np.uint8), size=(n, width))
        big_bc, tail_bc = barcodes(k_cells, 16), barcodes(5 * k_cells, 15)   # (another length: the tail's never equal a cell's)
        # names: (barcode row, 1..3 transcripts out of the cell's own 200, skewed towards its first ones)
        n_big = k_cells * per_cell
        tail_sizes = rng.integers(1, 6, 5 * k_cells)
        cell_of = np.concatenate([np.repeat(np.arange(k_cells), per_cell), k_cells + np.repeat(np.arange(5 * k_cells), tail_sizes)])
        n_names = len(cell_of)
        k_rows = rng.choice([1, 2, 3], size=n_names, p=[0.7, 0.2, 0.1])
        cell_base = rng.integers(0, n_tx - own, 6 * k_cells)
        row_name = np.repeat(np.arange(n_names), k_rows)
        pick = np.minimum((rng.random(len(row_name)) ** 2 * own).astype(np.int64), own - 1)
        tids = (cell_base[cell_of[row_name]] + pick).astype(np.uint32)
        order = rng.permutation(n_names)   # the cells' names interleaved, as a run leaves them

        def tables(keep):
            """the names `keep` (in the shuffled order) as row tables and records: one alignment a name, record = fixed fields + name"""
            sel = order[keep[order]]
            starts = np.concatenate([[0], np.cumsum(k_rows)])
            first = np.concatenate([[0], np.cumsum(k_rows[sel])[:-1]])   # the first row of every kept name among the kept rows
            rows = np.repeat(starts[sel] - first, k_rows[sel]) + np.arange(int(k_rows[sel].sum()))
            a = np.zeros((len(rows), 4), np.uint32)
            a[:, 0] = tids[rows]
            row_off = np.concatenate([[0], np.cumsum(k_rows[sel])]).astype(np.uint64)
            group_off = np.arange(len(sel) + 1, dtype=np.uint32)
            # [block_size][32 fixed bytes][name + NUL]; a cell's names are r_<16>_<UMI>, the tail's rx_<15>_<UMI>
            l_name = 2 + 16 + 1 + 8 + 1
            rec = np.zeros((len(rows), 36 + l_name), np.uint8)
            rec[:, 0] = 32 + l_name
            rec[:, 12] = l_name
            name = rec[:, 36:]
            cell = cell_of[np.repeat(sel, k_rows[sel])]
            is_big = cell < k_cells
            name[:, 0] = ord("r")
            name[is_big, 1] = ord("_")
            name[is_big, 2:18] = big_bc[cell[is_big]]
            name[~is_big, 1] = ord("x")
            name[~is_big, 2] = ord("_")
            name[~is_big, 3:18] = tail_bc[cell[~is_big] - k_cells]
            name[:, 18] = ord("_")
            name[:, 19:27] = np.frombuffer(b"ACGTACGT", np.uint8)
            rec_off = (np.arange(len(rows) + 1, dtype=np.uint64) * np.uint64(rec.shape[1]))
            return a, row_off, group_off, rec.reshape(-1), rec_off
        tx_feature = (np.arange(n_tx, dtype=np.uint32) // 2)
        out = {"config": "cells", "workload": "%d cells of %d read names + %d barcodes of 1-5 names, %d transcripts, %d genes, mode em" % (k_cells, per_cell, 5 * k_cells, n_tx, n_tx // 2)}
        keeps = {"all": np.ones(n_names, bool), "large": np.arange(n_names) < n_big, "tail": np.arange(n_names) >= n_big}
        for label, which, lds in (("all_default_lds", "all", None), ("all_lds_0", "all", 0), ("large_only_block_route", "large", None), ("tail_only_wave_route", "tail", None)):
            a, row_off, group_off, data, rec_off = tables(keeps[which])
            t = [torch.from_numpy(x).cuda() for x in (a.view(np.int32), row_off.view(np.int64), group_off.view(np.int32), data, rec_off.view(np.int64))]
            recs = lib.BrDeviceBam(t[3].data_ptr(), t[3].numel(), t[4].data_ptr(), t[4].numel() - 1)
            torch.cuda.synchronize()
            runs = []
            for step in range(args.warmup + args.steps):
                q = lib.Quant(n_tx)
                q.set_param("keep_names", 1)
                c = lib.Cells(mode=2, **({} if lds is None else {"lds_bytes": lds}))
                n_g = len(group_off) - 1
                for g0 in range(0, n_g, 1_000_000):
                    g1 = min(n_g, g0 + 1_000_000)
                    q.add_device(t[0], t[1], t[2], g0, g1)
                    c.add_device(t[1], t[2], recs, g0, g1)
                q.finish()
                n_c, n_z = c.finish(q, tx_feature, n_tx // 2)
                st = c.stats()
                iters = c.cell_stats()["iterations"]
                c.close()
                q.close()
                if step >= args.warmup:
                    runs.append({"add_s": round(st["add_us"] * 1e-6, 4), "finish_s": round(st["finish_us"] * 1e-6, 4), "values_kernel_s": round(st["values_us"] * 1e-6, 5),
                                 "cells": n_c, "matrix_entries": n_z, "names": st["names"], "entries": st["entries"], "pairs": st["pairs"], "slots": st["slots"],
                                 "wave_cells": st["wave_cells"], "block_cells": st["block_cells"], "hbm_cells": st["hbm_cells"],
                                 "iterations_mean": round(float(iters.mean()), 2), "iterations_max": int(iters.max())})
            out[label] = runs
            del t
        print(json.dumps(out))
        return
    if args.config == "collate":
        import ctypes as C
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe", with_records=1)
        stream, roff, rlen = synth.Annotation.frame_records(batch)
        del batch
        n_rec = len(roff)
        perm = np.random.default_rng(7).permutation(n_rec)   # an order that is not collated (a coordinate sort scatters names alike)
        d_blob = torch.from_numpy(stream).cuda()
        d_off = torch.from_numpy(roff[perm].astype(np.int64)).cuda()
        d_len = torch.from_numpy(rlen[perm].astype(np.int32)).cuda()
        torch.cuda.synchronize()
        runs = []
        for step in range(args.warmup + args.steps):
            c = lib.Collator(0)
            t0 = time.perf_counter()
            for a in range(0, n_rec, 1_000_000):
                c.add_device(d_blob, d_off[a:a + 1_000_000], d_len[a:a + 1_000_000])
            t1 = time.perf_counter()
            _, n_grp = c.finish()
            t2 = time.perf_counter()
            n_b = 0
            while c.next_records(1_000_000).n_aln:
                n_b += 1
            t3 = time.perf_counter()
            st = c.stats()
            c.close()
            if step >= args.warmup:
                runs.append({"add_s": round(t1 - t0, 4), "finish_s": round(t2 - t1, 4), "cut_s": round(t3 - t2, 4), "bundles": n_b,
                             "groups": n_grp, "arena_bytes_per_record": round(st["arena_bytes"] / n_rec, 1),
                             "peak_bytes_per_record": round(st["peak_bytes"] / n_rec, 1)})
        # the same stream split into records on the device without collating (the reader's split step, no inflate)
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        L = lib.lib()
        L.br_bam_split_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int32, C.c_void_p, C.POINTER(lib.BrDeviceRecords),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_uint64)]
        split = []
        for step in range(args.warmup + args.steps):
            recs, un, used = lib.BrDeviceRecords(), C.c_int64(), C.c_uint64()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lib.check(L.br_bam_split_device(ctx.h, C.c_void_p(d_blob.data_ptr()), stream.size, ann.n_refs, None, C.byref(recs), C.byref(un),
                                            C.byref(used)), "br_bam_split_device")
            torch.cuda.synchronize()
            if step >= args.warmup:
                split.append(round(time.perf_counter() - t0, 4))
        print(json.dumps({"config": "collate", "pairs": n, "records": n_rec, "stream_bytes": int(stream.size), "runs": runs,
                          "split_device_s": split}))
        return
    if args.config == "sort":
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        del batch
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        blob = torch.from_numpy(stream_h).to("cuda:0")
        off_d = torch.from_numpy(roff.view(np.int64)).to("cuda:0")
        len_d = torch.from_numpy(rlen.view(np.int32)).to("cuda:0")
        st = torch.cuda.current_stream().cuda_stream
        _, bam = ctx.project_bam_device(cfg, blob, off_d, len_d, np.arange(ann.flat["n_refs"], dtype=np.int32), st)
        torch.cuda.synchronize()
        n_rows, n_bytes = int(bam.n_rows), int(bam.n_bytes)
        # the deflate and the context's other calls reuse the context's buffers: the sorter works on a copy of the stream
        data = torch.as_tensor(brdev._DevArray(bam.data, n_bytes, "|u1"), device="cuda:0").clone()
        rows = torch.as_tensor(brdev._DevArray(bam.row_off, n_rows + 1, "<u8"), device="cuda:0").clone()
        torch.cuda.synchronize()
        runs = []
        for step in range(args.warmup + args.steps):
            s = lib.Sorter(0)
            t0 = time.perf_counter()
            for a in range(0, n_rows, 1_000_000):
                m = min(1_000_000, n_rows - a)
                s.add_device(lib.BrDeviceBam(data.data_ptr(), n_bytes, rows.data_ptr() + 8 * a, m), None)
            t1 = time.perf_counter()
            s.finish()
            t2 = time.perf_counter()
            pieces, z_bytes = 0, 0
            while True:
                p = s.next_records(128 << 20)
                if not p.n_rows:
                    break
                z = ctx.bgzf_deflate_device(torch.as_tensor(brdev._DevArray(p.data, int(p.n_bytes), "|u1"), device="cuda:0"), st)
                z_bytes += int(z.numel())
                pieces += 1
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            stt = s.stats()
            s.close()
            if step >= args.warmup:
                runs.append({"add_s": round(t1 - t0, 4), "finish_s": round(t2 - t1, 4), "drain_s": round(t3 - t2, 4),
                             "gather_s": round(stt["next_s"], 4), "pieces": pieces, "compressed_bytes": z_bytes,
                             "arena_bytes_per_record": round(stt["arena_bytes"] / n_rows, 1),
                             "peak_bytes_per_record": round(stt["peak_bytes"] / n_rows, 1)})
        print(json.dumps({"config": "sort", "pairs": n, "records": n_rows, "stream_bytes": n_bytes, "runs": runs}))
        return
    if args.config in ("quant", "quant_boot", "quant_genes"):
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe")
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        db = brdev.upload_batch(batch)
        goff = db["group_off"].cpu().numpy().view(np.uint32)
        n_aln, n_groups = int(db["n_aln"]), int(db["n_groups"])
        del batch
        n_tx = idx.num_transcripts()
        lens = np.asarray([idx.transcript_len(t) for t in range(n_tx)], dtype=np.int64)
        project = []
        for _ in range(2):   # (the second call runs on warm tables)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = ctx.project_batch_device(cfg, db)
            torch.cuda.synchronize()
            project.append(round(time.perf_counter() - t0, 4))
        n_rows = int(rows.n_rows)
        cuts = sorted(set(int(np.searchsorted(goff, a, side="left")) for a in range(0, n_aln, 1_000_000)) | {n_groups})   # names whose first alignment opens a slice
        if args.config == "quant_boot":
            runs = []
            for step in range(args.warmup + args.steps):
                q = lib.Quant(n_tx, lens)
                q.set_param("bootstraps", args.bootstraps)
                q.set_param("boot_seed", step)
                q.set_param("boot_chunk", args.boot_chunk)
                for g0, g1 in zip(cuts, cuts[1:]):
                    lib.check(q.add_raw(rows.a, rows.row_off, db["group_off"].data_ptr() + 4 * g0, g1 - g0, True), "br_quant_add")
                names, classes = q.finish()
                t0 = time.perf_counter()
                iters, _ = q.em()
                t1 = time.perf_counter()
                boot_iters = q.bootstrap()
                t2 = time.perf_counter()
                bs, stt = q.boot_stats(), q.stats()
                q.close()
                if step >= args.warmup:
                    point, boot = (t1 - t0) / max(iters, 1), bs["em_s"] / max(bs["iterations_total"], 1)
                    runs.append({"em_s": round(t1 - t0, 4), "iterations": iters, "em_us_per_replicate_iteration": round(1e6 * point, 2),
                                 "bootstrap_s": round(t2 - t1, 4), "boot_sample_s": round(bs["sample_s"], 4), "boot_em_s": round(bs["em_s"], 4),
                                 "boot_iterations_total": bs["iterations_total"], "boot_iterations_min": int(boot_iters.min()),
                                 "boot_iterations_max": int(boot_iters.max()), "boot_em_us_per_replicate_iteration": round(1e6 * boot, 2),
                                 "point_over_boot": round(point / boot, 2) if boot > 0 else None, "names": names, "classes": classes,
                                 "labels": stt["n_labels"], "peak_bytes": stt["peak_bytes"]})
            print(json.dumps({"config": "quant_boot", "pairs": n, "alignments": n_aln, "rows": n_rows, "transcripts": n_tx, "bootstraps": args.bootstraps,
                              "boot_chunk": args.boot_chunk, "runs": runs}))
            return
        if args.config == "quant_genes":
            tx_gene = np.ascontiguousarray(ann.flat["tx_gene"], dtype=np.uint32)
            n_genes = int(tx_gene.max()) + 1

            def timed(f):
                t0 = time.perf_counter()
                f()
                return round(time.perf_counter() - t0, 5)
            runs = []
            for step in range(args.warmup + args.steps):
                q = lib.Quant(n_tx, lens)
                q.set_param("bootstraps", args.bootstraps)
                q.set_param("boot_seed", step)
                for g0, g1 in zip(cuts, cuts[1:]):
                    lib.check(q.add_raw(rows.a, rows.row_off, db["group_off"].data_ptr() + 4 * g0, g1 - g0, True), "br_quant_add")
                names, classes = q.finish()
                q.em()
                q.genes(tx_gene, n_genes)
                gst, stt = q.gene_stats(), q.stats()
                run = {"finish_s": round(stt["finish_s"], 4), "genes_s": round(gst["seconds"], 4), "gene_result_s": timed(q.gene_result), "names": names,
                       "classes": classes, "labels": stt["n_labels"], "gene_classes": q.n_gene_classes, "gene_labels": gst["n_gene_labels"],
                       "held_bytes": stt["held_bytes"], "peak_bytes": stt["peak_bytes"]}
                if args.bootstraps:
                    q.bootstrap()
                    run.update({"boot_summary_s": timed(q.boot_summary), "gene_boot_summary_first_s": timed(q.gene_boot_summary),   # (the first call makes B x G)
                                "gene_boot_summary_s": timed(q.gene_boot_summary)})
                q.close()
                if step >= args.warmup:
                    runs.append(run)
            print(json.dumps({"config": "quant_genes", "pairs": n, "alignments": n_aln, "rows": n_rows, "transcripts": n_tx, "genes": n_genes,
                              "bootstraps": args.bootstraps, "runs": runs}))
            return
        runs, runs_eff = [], []
        for eff_len in (0, 1):   # 1: the fragment-length model, the adds through br_quant_add_rows (the CIGAR references and the pool as well)
            for step in range(args.warmup + args.steps):
                q = lib.Quant(n_tx, lens)
                q.set_param("eff_len", eff_len)
                t0 = time.perf_counter()
                for g0, g1 in zip(cuts, cuts[1:]):
                    if eff_len:
                        lib.check(q.add_rows_raw(rows.a, rows.cigar, rows.pool, rows.row_off, rows.n_rows, rows.n_pool_words,
                                                 db["group_off"].data_ptr() + 4 * g0, g1 - g0, True), "br_quant_add_rows")
                    else:
                        lib.check(q.add_raw(rows.a, rows.row_off, db["group_off"].data_ptr() + 4 * g0, g1 - g0, True), "br_quant_add")
                t1 = time.perf_counter()
                names, classes = q.finish()
                t2 = time.perf_counter()
                iters, rel = q.em()
                t3 = time.perf_counter()
                stt = q.stats()
                fld = q.fld() if eff_len else None
                q.close()
                if step >= args.warmup:
                    run = {"add_s": round(t1 - t0, 4), "add_ms_per_slice": round(1e3 * (t1 - t0) / (len(cuts) - 1), 3), "finish_s": round(t2 - t1, 4),
                           "em_s": round(t3 - t2, 4), "iterations": iters, "rel_change": rel, "em_us_per_iteration": round(1e6 * (t3 - t2) / max(iters, 1), 2),
                           "names": names, "unassigned": stt["n_unassigned"], "classes": classes, "labels": stt["n_labels"],
                           "peak_bytes_per_name": round(stt["peak_bytes"] / max(names, 1), 1)}
                    if eff_len:
                        run.update({k: fld[k] for k in ("n_obs", "n_no_fragment", "n_out_of_range")})
                        run["mean_fragment_length"] = round(float((np.arange(len(fld["hist"])) * fld["hist"].astype(np.float64)).sum()) / max(fld["n_obs"], 1), 2)
                    (runs_eff if eff_len else runs).append(run)
        print(json.dumps({"config": "quant", "pairs": n, "alignments": n_aln, "rows": n_rows, "transcripts": n_tx, "slices": len(cuts) - 1,
                          "project_s": project, "runs": runs, "runs_eff_length": runs_eff}))
        return
    if args.config == "coverage":
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe")
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        db = brdev.upload_batch(batch)
        n_aln, n_groups = int(db["n_aln"]), int(db["n_groups"])
        del batch
        n_tx = idx.num_transcripts()
        lens = np.asarray([idx.transcript_len(t) for t in range(n_tx)], dtype=np.int64)
        n_bases = int(np.maximum(lens, 0).sum())
        project = []
        for _ in range(2):   # (the second call runs on warm tables)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rows = ctx.project_batch_device(cfg, db)
            torch.cuda.synchronize()
            project.append(round(time.perf_counter() - t0, 4))
        n_rows = int(rows.n_rows)
        out = {"config": "coverage", "pairs": n, "alignments": n_aln, "rows": n_rows, "transcripts": n_tx, "bases": n_bases, "project_s": project}
        for key, step_rows in (("runs", n_rows), ("runs_sliced", 1_000_000)):
            runs = []
            for step in range(args.warmup + args.steps):
                c = lib.Coverage(lens)
                for r0 in range(0, n_rows, max(step_rows, 1)):
                    lib.check(c.add_rows_raw(rows.a, rows.cigar, rows.pool, rows.n_rows, rows.n_pool_words, r0, min(r0 + step_rows, n_rows), True),
                              "br_coverage_add_rows")
                n_runs = c.finish()
                stt, summ = c.stats(), c.summary()
                c.close()
                if step >= args.warmup:
                    runs.append({"add_s": round(stt["add_s"], 5), "finish_s": round(stt["finish_s"], 5), "adds": -(-n_rows // max(step_rows, 1)),
                                 "n_runs": n_runs, "rows_counted": stt["rows_counted"], "clipped_bases": stt["clipped_bases"],
                                 "aligned_bases": int(summ["aligned_bases"].sum()), "covered_bases": int(summ["covered_bases"].sum()),
                                 "max_depth": int(summ["max_depth"].max()) if n_tx else 0,
                                 "peak_bytes_per_base": round(stt["peak_bytes"] / max(n_bases, 1), 2)})
            out[key] = runs
        quant_add = []
        for step in range(args.warmup + args.steps):   # the comparison: the quantifier's add with the fragment pass, all names in one call
            q = lib.Quant(n_tx, lens)
            q.set_param("eff_len", 1)
            lib.check(q.add_rows_raw(rows.a, rows.cigar, rows.pool, rows.row_off, rows.n_rows, rows.n_pool_words, db["group_off"].data_ptr(), n_groups,
                                     True), "br_quant_add_rows")
            if step >= args.warmup:
                quant_add.append(round(q.stats()["add_s"], 5))
            q.close()
        out["quant_eff_len_add_s"] = quant_add
        print(json.dumps(out))
        return
    if args.config == "small":
        import subprocess
        root = os.path.dirname(os.path.abspath(__file__))
        ann = synth.Annotation("G")
        idx = lib.Index.from_flat(ann.flat, device=0)
        cfg = lib.make_config()
        out = {"config": "small", "unit": "us per call", "device_resident_step": {}}
        for pairs in (1, 32, 1000, 5000, 30000, 52000):
            batch = ann.reads(pairs, "pe", seed=1234 + pairs)
            db = brdev.upload_batch(batch, "cuda:0")
            row = {"alignments": int(batch["n_aln"])}
            for small in (1, 0):
                ctx = lib.Context(idx)
                ctx.set_param("small_batch", small)
                for _ in range(20):
                    ctx.project_batch_device(cfg, db, 0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                k = 300
                for _ in range(k):
                    ctx.project_batch_device(cfg, db, 0)
                torch.cuda.synchronize()
                row["no_host_round_trips" if small else "ordinary_pipeline"] = round((time.perf_counter() - t0) / k * 1e6, 1)
                ctx.close()
            out["device_resident_step"]["pairs=%d" % pairs] = row
        exe = "/tmp/group_latency"
        try:
            subprocess.check_call(["gcc", "-O2", "-std=c99", "-I", os.path.join(root, "include"), os.path.join(root, "profiles", "group_latency.c"),
                                   "-o", exe, "-L", os.path.join(root, "bramble_amd"), "-lbramble_amd", "-Wl,-rpath," + os.path.join(root, "bramble_amd")])
            runs = [json.loads(subprocess.run([exe], check=True, capture_output=True, text=True, timeout=300).stdout.strip().splitlines()[-1]) for _ in range(3)]
            out["host_to_host_from_c"] = {k: [r[k] for r in runs] for k in runs[0]}
        except Exception as e:   # no compiler on the box: the device-resident numbers stand alone
            out["host_to_host_from_c"] = "not measured: %s" % e
        print(json.dumps(out))
        return
    if args.config == "bam":
        # re-encode the rows of configs[1] as BAM records: HBM-bound byte streaming
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe", with_records=1)
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        pass
        if os.environ.get("BAM_LANES"):
            ctx.set_param("bam_lanes", int(os.environ["BAM_LANES"]))
        db = brdev.upload_batch(batch, "cuda:0")
        blob, roff = brdev.upload_records(batch, "cuda:0")
        stream = torch.cuda.current_stream().cuda_stream
        rows = ctx.project_batch_device(cfg, db, stream)
        n_rows = int(rows.n_rows)
        bam = ctx.bam_encode_device(cfg, blob, roff, stream)
        ctx.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kms = {}
        for _ in range(args.steps):
            bam = ctx.bam_encode_device(cfg, blob, roff, stream)
            for k, (ms, ln) in ctx.kernel_ms().items():
                kms[k] = kms.get(k, 0.0) + ms
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / args.steps
        out_bytes = int(bam.n_bytes)
        in_bytes_per_row = out_bytes  # every output byte is copied from (or computed next to) one input byte
        k_ms = kms.get("k_bam_scan+k_bam_size+k_bam_encode", 0.0) / args.steps
        print(json.dumps({"config": "bam", "workload": "re-encode the %d rows of %d paired-end alignments as BAM records" % (n_rows, batch["n_aln"]),
                          "rows_per_s": n_rows / el, "ms_per_step": el * 1e3, "output_bytes": out_bytes,
                          "input_record_bytes": int(len(batch["rec_blob"])), "kernel_ms_per_step": {k: round(v / args.steps, 3) for k, v in kms.items() if v},
                          "bam_kernels_GBps_read_plus_write": (out_bytes + in_bytes_per_row) / (k_ms * 1e-3) / 1e9 if k_ms else None,
                          "hbm_peak_GBps": 8000.0}))
        return
    if args.config == "bundle":
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        blob = torch.from_numpy(stream_h).to("cuda:0")
        off_d = torch.from_numpy(roff.view(np.int64)).to("cuda:0")
        len_d = torch.from_numpy(rlen.view(np.int32)).to("cuda:0")
        ref_map = np.arange(ann.flat["n_refs"], dtype=np.int32)
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(args.warmup):
            rows, bam = ctx.project_bam_device(cfg, blob, off_d, len_d, ref_map, st)
        ctx.set_profiling(True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kms = {}
        for _ in range(args.steps):
            rows, bam = ctx.project_bam_device(cfg, blob, off_d, len_d, ref_map, st)
            for k, (ms, ln) in ctx.kernel_ms().items():
                kms[k] = kms.get(k, 0.0) + ms
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / args.steps
        # optional last stage: BGZF deflate of the projected stream on the device
        if os.environ.get("DEFLATE_DYNAMIC") is not None:
            ctx.set_param("deflate_dynamic", int(os.environ["DEFLATE_DYNAMIC"]))
        z = ctx.bgzf_deflate_device(torch.as_tensor(brdev._DevArray(bam.data, int(bam.n_bytes), "|u1"), device="cuda:0"), st)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        zk = {}
        for _ in range(args.steps):
            z = ctx.bgzf_deflate_device(torch.as_tensor(brdev._DevArray(bam.data, int(bam.n_bytes), "|u1"), device="cuda:0"), st)
            for k, (ms, ln) in ctx.kernel_ms().items():
                zk[k] = zk.get(k, 0.0) + ms
        torch.cuda.synchronize()
        zel = (time.perf_counter() - t0) / args.steps
        deflate = {"ms_per_step": zel * 1e3, "compressed_bytes": int(z.numel()), "ratio": int(bam.n_bytes) / max(int(z.numel()), 1),
                   "GBps_in": int(bam.n_bytes) / zel / 1e9, "kernel_ms_per_step": {k: round(v / args.steps, 3) for k, v in zk.items() if v}}
        print(json.dumps({"config": "bundle", "device_deflate": deflate, "workload": "%d raw paired-end BAM records resident in HBM -> %d projected BAM records (reader side, projection and re-encoding on the device)" % (len(rlen), int(bam.n_rows)),
                          "alignments_per_s": len(rlen) / el, "ms_per_step": el * 1e3, "input_bytes": int(stream_h.size),
                          "output_bytes": int(bam.n_bytes), "kernel_ms_per_step": {k: round(v / args.steps, 3) for k, v in kms.items() if v}}))
        return
    if args.config == "samout":
        import subprocess
        import tempfile
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from tests import bamio
        n = args.reads or 500_000
        ann = synth.Annotation("G")
        annd = ann.as_dict()
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        del batch
        cfg = lib.make_config()
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        ctx.set_sam_refs([idx.transcript_name(t) for t in range(idx.num_transcripts())])
        blob = torch.from_numpy(stream_h).to("cuda:0")
        off_d = torch.from_numpy(roff.view(np.int64)).to("cuda:0")
        len_d = torch.from_numpy(rlen.view(np.int32)).to("cuda:0")
        ref_map = np.arange(ann.n_refs, dtype=np.int32)
        st = torch.cuda.current_stream().cuda_stream
        _, bam = ctx.project_bam_device(cfg, blob, off_d, len_d, ref_map, st)
        # the projected stream, copied out of the context's buffers (the calls below reuse them)
        recs = torch.as_tensor(brdev._DevArray(bam.data, int(bam.n_bytes), "|u1"), device="cuda:0").clone()
        rows = torch.as_tensor(brdev._DevArray(bam.row_off, int(bam.n_rows), "<u8"), device="cuda:0").view(torch.int64).clone()
        torch.cuda.synchronize()
        res = {"config": "samout", "workload": "SAM text of the %d projected records of %d paired-end alignments (%d record bytes) in HBM"
               % (int(bam.n_rows), len(rlen), int(bam.n_bytes))}
        ctx.set_profiling(True)
        for name, call in (("sam_format", lambda: ctx.sam_format_device(recs, rows, st)),
                           ("device_deflate", lambda: ctx.bgzf_deflate_device(recs, st))):
            for _ in range(args.warmup):
                out = call()
            times, kms = [], {}
            for _ in range(args.steps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = call()
                torch.cuda.synchronize()
                times.append(time.perf_counter() - t0)
                for k, (ms, ln) in ctx.kernel_ms().items():
                    kms[k] = kms.get(k, 0.0) + ms
            ms = 1e3 * float(np.median(times))
            res[name] = {"ms_per_bundle": round(ms, 3), "ms_min": round(1e3 * min(times), 3), "out_bytes": int(out.numel()),
                         "out_GBps": int(out.numel()) / (ms * 1e-3) / 1e9, "in_GBps": int(bam.n_bytes) / (ms * 1e-3) / 1e9,
                         "kernel_ms_per_step": {k: round(v / args.steps, 3) for k, v in kms.items() if v}}
        ctx.set_profiling(False)
        del recs, rows
        runs = int(os.environ.get("SAMOUT_CLI_RUNS", "3"))
        if runs:
            tmp = tempfile.mkdtemp(prefix="bramble_samout_")
            gtf, in_bam = os.path.join(tmp, "guides.gtf"), os.path.join(tmp, "in.bam")
            bamio.write_gtf(gtf, annd)
            refs = [(r, 250_000_000) for r in annd["refnames"]]
            bamio.write_bam(in_bam, "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs), refs, stream_h.tobytes(), level=1)
            exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bramble_amd", "bin", "bramble")
            import re
            wall, dev = {"bam": [], "sam": []}, {"bam": [], "sam": []}
            size = {}
            for k in range(runs):
                for fmt in ("bam", "sam"):
                    out = os.path.join(tmp, "out." + fmt)
                    t0 = time.perf_counter()
                    r = subprocess.run([exe, in_bam, "-G", gtf, "-o", out, "-p", str(args.threads), "-O", fmt], capture_output=True, timeout=600)
                    wall[fmt].append(time.perf_counter() - t0)
                    assert r.returncode == 0, r.stderr.decode()
                    dev[fmt].append(float(re.search(rb"([0-9.]+)s on the device path", r.stdout).group(1)))   # (the report line)
                    size[fmt] = os.path.getsize(out)
                    os.remove(out)
            res["cli_file_to_file_s"] = {f: {"median": round(float(np.median(v)), 3), "runs": [round(x, 3) for x in v], "out_bytes": size[f],
                                             "device_path_s": dev[f]} for f, v in wall.items()}
        print(json.dumps(res))
        return
    if args.config == "inflate":
        # BGZF inflate on the device against the host codec: the raw records of N read pairs, compressed by the library's writer
        import ctypes as C
        import tempfile
        n = args.reads or 10_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        L = lib.lib()
        L.br_bgzf_write_file.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int]
        L.br_bgzf_read_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.br_free_buffer.argtypes = [C.c_void_p]
        tmp = tempfile.mkdtemp(prefix="bramble_inflate_")
        path = os.path.join(tmp, "records.bgzf")
        assert L.br_bgzf_write_file(path.encode(), stream_h.ctypes.data, stream_h.size, args.threads, 6) == 0
        raw = np.fromfile(path, dtype=np.uint8)
        t0 = time.perf_counter()
        blocks, consumed, total = lib.bgzf_scan(raw)
        scan_s = time.perf_counter() - t0
        assert consumed == raw.size and total == stream_h.size
        idx = lib.Index.from_flat(ann.flat, device=0)
        ctx = lib.Context(idx)
        src = torch.from_numpy(raw).to("cuda:0")
        out = ctx.bgzf_inflate_device(src, blocks)
        assert torch.equal(out.cpu(), torch.from_numpy(stream_h))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = ctx.bgzf_inflate_device(src, blocks)
        torch.cuda.synchronize()
        el = (time.perf_counter() - t0) / args.steps
        host = {}
        for th in (1, args.threads):
            p, nb = C.c_void_p(), C.c_uint64()
            t0 = time.perf_counter()
            assert L.br_bgzf_read_file(path.encode(), th, C.byref(p), C.byref(nb)) == 0
            host["threads=%d" % th] = round(time.perf_counter() - t0, 3)
            L.br_free_buffer(p)
        print(json.dumps({"config": "inflate", "workload": "%d BAM records, %d bytes in %d BGZF blocks of %d compressed bytes (host writer, level 6)" % (len(rlen), total, len(blocks), raw.size),
                          "device_ms": el * 1e3, "device_GBps_out": total / el / 1e9, "device_GBps_in": raw.size / el / 1e9, "block_scan_host_s": round(scan_s, 3),
                          "host_whole_file_s (br_bgzf_read_file, includes its buffer growth)": host, "kernel_ms": {k: round(v[0], 3) for k, v in ctx.kernel_ms().items() if v[0]}}))
        return
    if args.config == "sam":
        import subprocess
        import tempfile
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from tests import bamio
        n = args.reads or 2_000_000
        ann = synth.Annotation("G")
        annd = ann.as_dict()
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        refs = [(r, 250_000_000) for r in annd["refnames"]]
        header = "@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)
        text = synth.records_to_sam(stream_h, annd["refnames"])
        tmp = os.environ.get("CLI_TMP") or tempfile.mkdtemp(prefix="bramble_sam_")
        os.makedirs(tmp, exist_ok=True)
        gtf, in_sam, in_bam = os.path.join(tmp, "guides.gtf"), os.path.join(tmp, "in.sam"), os.path.join(tmp, "in.bam")
        bamio.write_gtf(gtf, annd)
        with open(in_sam, "wb") as f:
            f.write(header.encode())
            f.write(text)
        bamio.write_bam(in_bam, header, refs, stream_h.tobytes(), level=1)
        # device parse: the text in chunks of the command line's size (1 M records' worth), warmup first
        chunk = int(len(text) / max(len(rlen), 1) * 1_000_000)
        r = lib.SamReader(header)
        for _ in range(args.warmup):
            r.next(text[:text.rfind(b"\n", 0, chunk) + 1], True, fetch=False)
        s0 = r.stats()
        n_rec = 0
        for _ in range(args.steps):
            pos = 0
            while pos < len(text):
                got = r.next(text[pos:pos + chunk], pos + chunk >= len(text), fetch=False)
                pos += got["consumed"]
                n_rec += got["n"] + got["n_unmapped"]
        s1 = r.stats()
        r.close()
        parse_s, up_s, nch, nb = s1["parse_s"] - s0["parse_s"], s1["upload_s"] - s0["upload_s"], s1["chunks"] - s0["chunks"], s1["bytes"] - s0["bytes"]
        exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bramble_amd", "bin", "bramble")
        walls = {}
        for label, path in (("bam", in_bam), ("sam", in_sam), ("bam'", in_bam), ("sam'", in_sam)):   # alternated, twice
            out = os.path.join(tmp, "out_%s.bam" % label.strip("'"))
            t0 = time.perf_counter()
            p = subprocess.run([exe, path, "-G", gtf, "-o", out, "-p", str(args.threads)], capture_output=True, text=True)
            if p.returncode != 0:
                print(p.stderr, file=sys.stderr)
                sys.exit(1)
            walls[label] = round(time.perf_counter() - t0, 3)
        print(json.dumps({"config": "sam", "workload": "%d paired-end alignments as SAM text (%.2f GB), %d chunks of ~%.0f MB" % (len(rlen), len(text) / 1e9, nch / max(args.steps, 1), chunk / 1e6),
                          "device_parse_ms_per_chunk": round(1e3 * parse_s / max(nch, 1), 2), "text_GBps_parse": round(nb / parse_s / 1e9, 1),
                          "records_per_s_parse": round(n_rec / parse_s), "text_GBps_upload": round(nb / up_s / 1e9, 1),
                          "cli_wall_s": walls, "sam_bytes": len(text), "bam_bytes": os.path.getsize(in_bam)}))
        return
    if args.config == "cli":
        pass
        import subprocess
        import tempfile
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        from tests import bamio
        n = args.reads or 2_000_000
        ann = synth.Annotation("G")
        annd = ann.as_dict()
        batch = ann.reads(n, "pe", with_records=1)
        stream_h, roff, rlen = synth.Annotation.frame_records(batch)
        tmp = os.environ.get("CLI_TMP") or tempfile.mkdtemp(prefix="bramble_cli_")   # CLI_TMP: keep guides.gtf / in.bam where a profiler run finds them
        os.makedirs(tmp, exist_ok=True)
        gtf, in_bam = os.path.join(tmp, "guides.gtf"), os.path.join(tmp, "in.bam")
        bamio.write_gtf(gtf, annd)
        refs = [(r, 250_000_000) for r in annd["refnames"]]
        t0 = time.perf_counter()
        # input preparation (not measured): BAM header + the framed records, BGZF-compressed with the library's writer
        import ctypes as C
        import struct
        text = ("@HD\tVN:1.6\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs)).encode()
        hb = bytearray(b"BAM\x01" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs)))
        for name, ln in refs:
            nm = name.encode() + b"\0"
            hb += struct.pack("<i", len(nm)) + nm + struct.pack("<i", ln)
        whole = np.concatenate([np.frombuffer(bytes(hb), dtype=np.uint8), stream_h])
        L = lib.lib()
        L.br_bgzf_write_file.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int]
        assert L.br_bgzf_write_file(in_bam.encode(), whole.ctypes.data, whole.size, args.threads, 6) == 0
        del whole
        prep = time.perf_counter() - t0
        exe = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bramble_amd", "bin", "bramble")
        res = {}
        # CLI_LEVELS entries: a host codec level or "device", optionally "@NAME=VALUE[@...]" environment for that run (A/B on one input)
        for entry in os.environ.get("CLI_LEVELS", "1,6,device").split(","):
            parts = entry.split("@")
            level = parts[0] if parts[0] == "device" else int(parts[0])
            run_env = dict(os.environ)
            run_env.update(dict(kv.split("=", 1) for kv in parts[1:] if not kv.startswith("ARG=")))
            entry_args = [kv[4:] for kv in parts[1:] if kv.startswith("ARG=")]   # "@ARG=--host-reader": an extra command-line argument for that run
            os.sync()   # the previous run's output is on its way to the disk: not this run's business
            time.sleep(float(os.environ.get("CLI_GAP_S", "0")))   # ... and the driver is still taking the previous process apart
            out_bam = os.path.join(tmp, "out%s.bam" % level)
            if os.path.exists(out_bam):
                os.remove(out_bam)
            t0 = time.perf_counter()
            e0 = time.time()
            import resource
            ru0 = resource.getrusage(resource.RUSAGE_CHILDREN)
            codec = ["--device-deflate"] if level == "device" else ["--compression-level", str(level)]
            extra = os.environ.get("CLI_EXTRA", "").split()
            r = subprocess.run([exe, in_bam, "-G", gtf, "-o", out_bam, "-p", str(args.threads)] + codec + extra + entry_args,
                               capture_output=True, text=True, env=run_env)
            wall = time.perf_counter() - t0
            e1 = time.time()
            if os.environ.get("BRAMBLE_AMD_TIMING"):
                print("%s: spawn at %.3f, child gone at %.3f\n%s" % (entry, e0, e1, r.stderr), file=sys.stderr)
            if r.returncode != 0:
                print(r.stderr, file=sys.stderr)
                sys.exit(1)
            tail = [l for l in r.stdout.splitlines() if "bundles" in l or "stage busy" in l or "release of" in l]
            key = "level%s" % entry
            while key in res:
                key += "'"
            ru1 = resource.getrusage(resource.RUSAGE_CHILDREN)
            import xxhash
            hx = xxhash.xxh64()
            with open(out_bam, "rb") as fh:
                for blk in iter(lambda: fh.read(1 << 24), b""):
                    hx.update(blk)
            rec_hash = None
            if os.environ.get("CLI_VERIFY"):   # the inflated record stream (whatever the bundle cuts and the BGZF framing were)
                L.br_bgzf_read_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
                L.br_free_buffer.argtypes = [C.c_void_p]
                pp, nn = C.c_void_p(), C.c_uint64()
                assert L.br_bgzf_read_file(out_bam.encode(), args.threads, C.byref(pp), C.byref(nn)) == 0
                view = (C.c_uint8 * nn.value).from_address(pp.value)
                hr = xxhash.xxh64()
                mv = memoryview(view)
                for q in range(0, nn.value, 1 << 26):
                    hr.update(mv[q:q + (1 << 26)])
                rec_hash = hr.hexdigest()
                del mv, view
                L.br_free_buffer(pp)
            res[key] = {"out_xxh64": hx.hexdigest(), "inflated_xxh64": rec_hash, "wall_s": round(wall, 2), "user_s": round(ru1.ru_utime - ru0.ru_utime, 2), "sys_s": round(ru1.ru_stime - ru0.ru_stime, 2),
                        "max_rss_gb": round(ru1.ru_maxrss / 1048576.0, 2), "alignments_per_s": len(rlen) / wall, "out_bam_bytes": os.path.getsize(out_bam),
                                       "report": " | ".join(tail)}
        print(json.dumps({"config": "cli", "workload": "%d paired-end alignments, BAM file -> BAM file, -p %d, GENCODE-shaped GTF (%d transcripts)" % (len(rlen), args.threads, len(annd["transcripts"])),
                          "in_bam_bytes": os.path.getsize(in_bam), "uncompressed_in_bytes": int(stream_h.size), "results": res,
                          "input_prep_s": round(prep, 1)}))
        return
    if args.config == "c5":
        n = args.reads or 1_000_000
        ann = synth.Annotation("G")
        batch = ann.reads(n, "hifi")
        cfg = lib.make_config(lr_hq=1, strict=1, sim_thr=0.95)
        label = "%d HiFi-like reads (median 2 kb) --lr-hq --strict --similarity-threshold 0.95 vs GENCODE-shaped annotation" % n
    else:
        n = args.reads or 200_000
        ann = synth.Annotation("G", n_genes=6000, n_refs=5, with_genome=True)
        batch = ann.reads(n, "ont", with_seq=1)
        cfg = lib.make_config(lr=1, use_fasta=1)
        label = "%d ONT-like reads (median 900 bp, clips <= 300) --lr -S vs a 6000-gene annotation with synthetic genome" % n
    idx = lib.Index.from_flat(ann.flat, device=0)
    ctx = lib.Context(idx)
    if os.environ.get("KSW_FAST") is not None:
        ctx.set_param("ksw_fast", int(os.environ["KSW_FAST"]))
    if os.environ.get("KSW_TAPE_MB") is not None:
        ctx.set_param("ksw_tape_mb", int(os.environ["KSW_TAPE_MB"]))
    db = brdev.upload_batch(batch, "cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(args.warmup):
        rows = ctx.project_batch_device(cfg, db, stream)
    ctx.set_profiling(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kms = {}
    for _ in range(args.steps):
        rows = ctx.project_batch_device(cfg, db, stream)
        for k, (ms, ln) in ctx.kernel_ms().items():
            kms[k] = kms.get(k, 0.0) + ms
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    out = {"config": args.config, "workload": label, "alignments_per_step": int(batch["n_aln"]),
           "value": batch["n_aln"] * args.steps / el, "unit": "alignments/s", "ms_per_step": 1e3 * el / args.steps,
           "projected_records": int(rows.n_rows), "matches": int(rows.n_matches),
           "kernel_ms_per_step": {k: round(v / args.steps, 3) for k, v in kms.items() if v}}
    if args.config == "c3":
        st = ctx.rescue_stats()
        ksw_ms = kms.get("k_ksw", 0.0) / args.steps
        out["rescue"] = st
        out["ksw_routing"] = ctx.ksw_diag()
        out["k_ksw_GCUPS"] = st["dp_cells"] / (ksw_ms * 1e-3) / 1e9 if ksw_ms else None
    print(json.dumps(out))


if __name__ == "__main__":
    sys.exit(main())

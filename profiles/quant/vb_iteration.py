"""The cost of one variational Bayes iteration of br_quant beside one plain EM iteration, on the class table the 10 M-pair
benchmark workload produces (bench_extra.py quant's input: the synthetic-input tool's annotation "G" and its paired reads,
projected on the device).  Both run a fixed 320 iterations ("tolerance" 0) and are timed by br_quant_stats' EM seconds; the two
estimators alternate, the first round warms up and is not reported.  With --bootstraps B the replicates (the same 320
iterations each) are timed the same way, per replicate and iteration.  One JSON line.

    python profiles/quant/vb_iteration.py [--reads N] [--rounds R] [--bootstraps B]
    rocprofv3 --kernel-trace --stats -- python profiles/quant/vb_iteration.py --rounds 1     # where the time goes"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

ITERS = 320


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bootstraps", type=int, default=0)
    args = ap.parse_args()
    import torch
    from bramble_amd import device as brdev, lib, synth
    ann = synth.Annotation("G")
    batch = ann.reads(args.reads, "pe")
    idx = lib.Index.from_flat(ann.flat, device=0)
    ctx = lib.Context(idx)
    db = brdev.upload_batch(batch)
    del batch
    n_tx = idx.num_transcripts()
    lens = np.asarray([idx.transcript_len(t) for t in range(n_tx)], dtype=np.int64)
    rows = ctx.project_batch_device(lib.make_config(), db)
    torch.cuda.synchronize()
    out = {"pairs": args.reads, "transcripts": n_tx, "iterations": ITERS, "em_us": [], "vb_us": [], "boot_em_us": [], "boot_vb_us": []}
    for rnd in range(args.rounds + 1):
        for vb in (0, 1):
            q = lib.Quant(n_tx, lens, vb=vb)
            q.set_param("max_iters", ITERS)
            q.set_param("tolerance", 0)
            if args.bootstraps:
                q.set_param("bootstraps", args.bootstraps)
            lib.check(q.add_raw(rows.a, rows.row_off, db["group_off"].data_ptr(), int(db["n_groups"]), True), "br_quant_add")
            out["names"], out["classes"] = q.finish()
            assert q.em()[0] == ITERS
            st = q.stats()
            out["labels"] = st["n_labels"]
            if args.bootstraps:
                q.bootstrap()
                bs = q.boot_stats()
            q.close()
            if rnd:
                out["vb_us" if vb else "em_us"].append(round(1e6 * st["em_s"] / ITERS, 2))
                if args.bootstraps:
                    out["boot_vb_us" if vb else "boot_em_us"].append(round(1e6 * bs["em_s"] / max(bs["iterations_total"], 1), 2))
    for key in ("em_us", "vb_us", "boot_em_us", "boot_vb_us"):
        if out[key]:
            out[key + "_median"] = float(np.median(out[key]))
    out["vb_over_em"] = round(out["vb_us_median"] / out["em_us_median"], 3)
    if args.bootstraps:
        out["boot_vb_over_em"] = round(out["boot_vb_us_median"] / out["boot_em_us_median"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

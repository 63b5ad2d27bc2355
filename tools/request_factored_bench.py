#!/usr/bin/env python3
"""Factored request-form batches on one MI355X -> profiles/request_factored.json.

  submit   host clock per block with the pinned buffers already filled: fr_worker_submit_requests_factored + sync against fr_worker_submit_requests
           + sync on the same worker and the same block, ALTERNATING, `--rounds` rounds of `--blocks` blocks a side after a warm-up of both; per
           side the median of the rounds' medians and their spread (min .. max), the ratio of the two medians, and the largest score difference
           over the largest score.  Configurations (full-size tables): Model-A fp32 at batch 256 and 4096 with 20 of the 47 columns shared and 16
           candidates per request; Model-C per bank bf16 at batch 4096 with half of the index columns shared, at 1 and at 16 requests per block.
  trace    (--leg trace, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/request_factored_bench.py --leg trace`): the same
           configurations, `--blocks` factored blocks each and nothing else, so that the trace's per-kernel statistics give the times of
           reqfc_user_kernel and reqfc_cand_kernel alone.  Writes nothing itself.

    python tools/request_factored_bench.py [--leg submit|trace] [--rounds 7] [--blocks 200] [--out profiles/request_factored.json]
    --rehearse: the CPU back-end, row-capped tables, small counts: checks the plumbing; its times are not measurements and the file says so.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = (   # name, model, index mode, precision, batch, requests per block, shared columns (None: half)
    ("A-256-f32", "A", None, "f32", 256, 16, 20),
    ("A-4096-f32", "A", None, "f32", 4096, 256, 20),
    ("C-4096-bf16-1req", "C", "bank", "bf16", 4096, 1, None),
    ("C-4096-bf16-16req", "C", "bank", "bf16", 4096, 16, None),
)


def setup(fr, args, cfg):
    name, which, mode, prec, batch, n_req, n_shared = cfg
    m = fr.Model.builtin(fr.MODEL_A if which == "A" else fr.MODEL_C)
    kw = {"index_mode": fr.INDEX_PER_BANK} if mode == "bank" else {}
    if args.rehearse:
        kw["max_rows"] = 200
    if kw:
        m = m.clone(**kw)
    ctx = fr.Context(m, device=-1 if args.rehearse else 0)
    ctx.fill_tables(fr.FILL_HASH, 7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
    if prec == "bf16" and not args.rehearse:
        ctx.set_fc_precision(fr.FC_BF16)
    C = m.idx_cols
    shared = (np.arange(C) < (n_shared if n_shared is not None else C // 2)).astype(np.int32)
    ctx.set_request_columns(shared, False)
    wk = fr.Worker(ctx, batch)
    rng = np.random.default_rng(91)
    ranges = np.asarray(m.index_ranges(), np.float64)
    rows = lambda n, cols: (rng.random((n, int(cols.sum()))) * ranges[cols][None, :]).astype(np.int32)
    req, cand = rows(n_req, shared.astype(bool)), rows(batch, ~shared.astype(bool))
    dense = rng.standard_normal((batch, m.dense_len)).astype(np.float32) if m.dense_len else None
    off = (np.arange(n_req + 1) * (batch // n_req)).astype(np.int32)
    wk._load_requests(req, cand, off, None, dense, None, None, 0)   # the pinned buffers, filled once: both forms read them in place
    return ctx, wk, batch, n_req


def leg_submit(fr, args):
    out = []
    for cfg in CONFIGS:
        ctx, wk, batch, n_req = setup(fr, args, cfg)
        sides = {"factored": lambda: wk.submit_requests_factored(batch, n_req), "full_rows": lambda: wk.submit_requests(batch, n_req, 0)}
        scores, med = {}, {k: [] for k in sides}
        for k, call in sides.items():   # warm-up of both (code objects, split images), and the scores of either side
            for _ in range(20):
                call()
                wk.sync()
            scores[k] = wk.score[:batch].astype(np.float64).copy()
        for _ in range(args.rounds):
            for k, call in sides.items():
                t = []
                for _ in range(args.blocks):
                    t0 = time.perf_counter()
                    call()
                    wk.sync()
                    t.append(time.perf_counter() - t0)
                med[k].append(1e6 * float(np.median(t)))
        r = {"config": cfg[0], "batch": batch, "requests": n_req, "kernel": wk.last_kernel(),
             "score_diff_over_max": float(np.abs(scores["factored"] - scores["full_rows"]).max() / np.abs(scores["full_rows"]).max())}
        for k in sides:
            r[k + "_us"] = {"median": float(np.median(med[k])), "min": min(med[k]), "max": max(med[k]), "rounds": med[k]}
        r["factored_over_full_rows"] = r["factored_us"]["median"] / r["full_rows_us"]["median"]
        print(json.dumps({k: v for k, v in r.items() if not k.endswith("_us")}), r["factored_us"]["median"], r["full_rows_us"]["median"], flush=True)
        out.append(r)
        wk.close()
        ctx.close()
    return out


def leg_trace(fr, args):
    for cfg in CONFIGS:
        ctx, wk, batch, n_req = setup(fr, args, cfg)
        for _ in range(args.blocks):
            wk.submit_requests_factored(batch, n_req)
            wk.sync()
        wk.close()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="submit", choices=("submit", "trace"))
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--blocks", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "request_factored.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as graft
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("request_factored_bench: no MI355X visible -- a timing needs the GPU")
    if args.leg == "trace":
        return leg_trace(fr, args)
    doc = {"tool": "tools/request_factored_bench.py", "rehearsal_not_a_measurement": bool(args.rehearse), "rounds": args.rounds, "blocks_per_round": args.blocks,
           "clock": "host clock around submit + sync, pinned buffers filled; the two sides alternate round by round", "submit": leg_submit(fr, args)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

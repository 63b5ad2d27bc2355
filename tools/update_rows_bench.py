#!/usr/bin/env python3
"""Sparse row updates against the only route the library had before them, in one process on one MI355X -> profiles/update_rows.json.

Model-C (full size), FR_INDEX_PER_BANK, bf16 chain (the per-bank operand-type bank image in place), one HBM table (the one with the most rows).
For n = 1 000, 10 000 and 100 000 distinct random rows per call, after warm-up, `--reps` (>= 20) repetitions each, medians (and min / max):
  (a) update_host_ms    fr_ctx_update_rows from host arrays: host clock around the call (it is synchronous);
  (b) update_worker_ms  fr_worker_update_rows from device arrays: host clock from the enqueue to the end of fr_worker_sync;
  (c) next_push_ms      the next batch-4096 fr_worker_push_device after the update, until fr_worker_sync has its scores (host clock);
and beside them the old route with the same rows: fr_ctx_upload_table, one call per contiguous run of row ids (upload_ms, with the
number of runs), and the next batch-4096 push, which pays the rebuild of the whole image (next_push_after_upload_ms).  The image's build
count is read around every leg: 0 builds under the updates, one per upload round.
--kernels (default on a GPU): per n, a fresh child process of this tool under `rocprofv3 --kernel-trace --stats` (a run of its own: the
times above are taken with the profiler off) enqueues the same updates; the kernel times are the medians over its LAST `reps` dispatches of
fill_table_kernel (the scatter arm) and convert_rows_lp_kernel<1> (the listed-rows arm) -- the procedural fill and the image build at the
head of the run are dispatches of the same two kernels and are left out that way.  Achieved bytes/s = the bytes the update must move
(scatter: n x dim x 4 read + written, + 4 n of ids; patch: n x dim x 4 read, n x dim x 2 written, + 4 n of ids) over the kernel time.

    python tools/update_rows_bench.py [--n 1000,10000,100000] [--reps 20] [--out profiles/update_rows.json] [--trace-dir build/update_rows_trace]
    --rehearse: tiny tables on the CPU back-end, fp32, no kernels: the plumbing only (its times are not measurements and the file says so).
"""
import argparse
import ctypes
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SEED_TABLES, SEED_WEIGHTS, BATCH, WARMUP = 0xF1EE7, 99, 4096, 3


def setup(fr, device, rehearse):
    base = fr.Model.builtin(fr.MODEL_C)
    model = base.clone(max_rows=20000, index_mode=fr.INDEX_PER_BANK) if rehearse else base.clone(index_mode=fr.INDEX_PER_BANK)
    ctx = fr.Context(model, device=device)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    if not rehearse:
        ctx.set_fc_precision(fr.FC_BF16)
    tabs = model.tables()
    hbm = [t for t, d in enumerate(tabs) if d.mem_class == 0] or list(range(len(tabs)))
    table = max(hbm, key=lambda t: tabs[t].rows)
    wk = fr.Worker(ctx, BATCH)
    rng = np.random.default_rng(2610)
    ranges = model.index_ranges()
    idx = (rng.random((BATCH, len(ranges))) * ranges[None, :]).astype(np.int32)
    dense = rng.standard_normal((BATCH, model.dense_len)).astype(np.float32) if model.dense_len else None
    bufs = (fr.DeviceBuffer.from_numpy(ctx, idx), fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None, fr.DeviceBuffer(ctx, BATCH * 4))
    return model, ctx, wk, table, bufs, rng


def push(wk, bufs):
    t0 = time.perf_counter()
    wk.push_device(BATCH, bufs[0], bufs[1], bufs[2])
    wk.sync()
    return (time.perf_counter() - t0) * 1e3


def stat(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "reps": len(xs)}


def runs_of(ids):
    """contiguous runs [start, start + len) of the sorted ids, and for each the positions of its rows in the id list"""
    order = np.argsort(ids, kind="stable")
    s = ids[order]
    cut = np.flatnonzero(np.diff(s) != 1) + 1
    return [(int(seg[0]), order[a:a + len(seg)]) for a, seg in zip(np.concatenate(([0], cut)), np.split(s, cut))]


def measure(fr, args, device, rehearse):
    model, ctx, wk, table, bufs, rng = setup(fr, device, rehearse)
    d = model.tables()[table]
    rows, dim = int(d.rows), d.dim
    out = {"table": table, "table_rows": rows, "table_dim": dim, "per_n": {}}
    push(wk, bufs)   # the first image
    L, h = fr.lib(), ctx._h
    for n in args.n:
        n = min(n, rows)
        ids = rng.permutation(rows)[:n].astype(np.int32)
        new = rng.standard_normal((n, dim)).astype(np.float32)
        d_ids, d_new = fr.DeviceBuffer.from_numpy(ctx, ids), fr.DeviceBuffer.from_numpy(ctx, new)
        runs = [(r0, np.ascontiguousarray(new[pos])) for r0, pos in runs_of(ids)]
        legs = {k: [] for k in ("update_host_ms", "next_push_after_host_update_ms", "update_worker_ms", "next_push_ms", "upload_ms", "next_push_after_upload_ms")}
        builds0 = ctx.lp_bank_image_builds()
        for rep in range(WARMUP + args.reps):
            keep = rep >= WARMUP
            t0 = time.perf_counter()
            ctx.update_rows(table, ids, new)
            t1 = time.perf_counter()
            p_a = push(wk, bufs)
            t2 = time.perf_counter()
            wk.update_rows(table, n, d_ids, d_new)
            wk.sync()
            t3 = time.perf_counter()
            p_b = push(wk, bufs)
            if keep:
                legs["update_host_ms"].append((t1 - t0) * 1e3)
                legs["next_push_after_host_update_ms"].append(p_a)
                legs["update_worker_ms"].append((t3 - t2) * 1e3)
                legs["next_push_ms"].append(p_b)
        builds_updates = ctx.lp_bank_image_builds() - builds0
        for rep in range(WARMUP + args.reps):
            t0 = time.perf_counter()
            for r0, block in runs:
                fr._check(L.fr_ctx_upload_table(h, table, r0, block.shape[0], block.ctypes.data_as(ctypes.c_void_p)))
            t1 = time.perf_counter()
            p = push(wk, bufs)
            if rep >= WARMUP:
                legs["upload_ms"].append((t1 - t0) * 1e3)
                legs["next_push_after_upload_ms"].append(p)
        rec = {k: stat(v) for k, v in legs.items()}
        rec.update({"n": n, "contiguous_runs": len(runs), "image_builds_during_update_legs": builds_updates,
                    "image_builds_during_upload_legs": ctx.lp_bank_image_builds() - builds0 - builds_updates,
                    "scatter_bytes": n * dim * 8 + 4 * n, "patch_bytes": n * dim * 6 + 4 * n})
        out["per_n"][str(n)] = rec
        print("n=%6d: host form %.3f ms, worker form %.3f ms, next push %.3f ms | upload route (%d runs) %.3f ms, next push %.3f ms" % (
            n, rec["update_host_ms"]["median"], rec["update_worker_ms"]["median"], rec["next_push_ms"]["median"], len(runs), rec["upload_ms"]["median"],
            rec["next_push_after_upload_ms"]["median"]), flush=True)
        d_ids.free()
        d_new.free()
    wk.close()
    ctx.close()
    return out


def traced_child(fr, args, device):
    """the run rocprofv3 watches: one n, WARMUP + reps worker-form updates with the image in place"""
    model, ctx, wk, table, bufs, rng = setup(fr, device, False)
    d = model.tables()[table]
    n = min(args.n[0], int(d.rows))
    push(wk, bufs)
    ids = rng.permutation(int(d.rows))[:n].astype(np.int32)
    d_ids, d_new = fr.DeviceBuffer.from_numpy(ctx, ids), fr.DeviceBuffer.from_numpy(ctx, rng.standard_normal((n, d.dim)).astype(np.float32))
    for _ in range(WARMUP + args.reps):
        wk.update_rows(table, n, d_ids, d_new)
        wk.sync()
    wk.close()
    ctx.close()


def kernel_times(args, n):
    tdir = os.path.join(args.trace_dir, "n%d" % n)
    os.makedirs(tdir, exist_ok=True)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tdir, "--", sys.executable, os.path.abspath(__file__), "--child", "--n", str(n),
           "--reps", str(args.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    traces = glob.glob(os.path.join(tdir, "**", "*kernel_trace.csv"), recursive=True)
    if p.returncode != 0 or not traces:
        return {"error": "rocprofv3 run failed (status %d)" % p.returncode, "tail": p.stdout.decode(errors="replace")[-600:]}
    by = {}
    for r in csv.DictReader(open(traces[0])):
        name = r["Kernel_Name"].split("(")[0].replace("void ", "").strip()
        if name.startswith(("fill_table_kernel", "convert_rows_lp_kernel")):
            by.setdefault(name, []).append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    out = {}
    for name, ev in by.items():
        last = [dur / 1e3 for _, dur in sorted(ev)[-args.reps:]]
        out[name] = {"median_us": statistics.median(last), "min_us": min(last), "max_us": max(last), "dispatches_taken": len(last), "dispatches_in_run": len(ev)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000,10000,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_rows.json"))
    ap.add_argument("--trace-dir", default=os.path.join(ROOT, "build", "update_rows_trace"))
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    args.n = [int(v) for v in args.n.split(",")]
    fr = graft.load_package()
    if args.child:
        traced_child(fr, args, 0)
        return
    if args.reps < 20 and not args.rehearse:
        sys.exit("--reps below 20 is not a measurement")
    t0 = time.time()
    res = {"tool": "tools/update_rows_bench.py", "model": "Model-C, FR_INDEX_PER_BANK, " + ("fp32 on the CPU back-end, row-capped" if args.rehearse else "bf16 chain, full size"),
           "batch": BATCH, "warmup": WARMUP, "reps": args.reps, "timing": "host clock around calls that end in a synchronise; medians",
           "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse)}
    kern = {}
    if not args.rehearse and not args.no_kernels:   # first: children of a parent that has not opened the GPU yet
        for n in args.n:
            kern[str(n)] = kernel_times(args, n)
            print("n=%d kernels: %s" % (n, json.dumps(kern[str(n)])), flush=True)
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("update_rows_bench.py measures on an MI355X: no HIP device is visible (--rehearse checks the plumbing on the CPU back-end)")
    res.update(measure(fr, args, fr.DEVICE_CPU if args.rehearse else 0, args.rehearse))
    for n, k in kern.items():
        rec = res["per_n"].get(n)
        if rec is None:
            continue
        rec["kernels_rocprofv3"] = k
        for name, byts in (("fill_table_kernel", rec["scatter_bytes"]), ("convert_rows_lp_kernel<1>", rec["patch_bytes"])):
            if name in k:
                k[name]["achieved_GBps"] = byts / (k[name]["median_us"] * 1e-6) / 1e9
    res["wall_s"] = time.time() - t0
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote %s" % args.out)


if __name__ == "__main__":
    main()

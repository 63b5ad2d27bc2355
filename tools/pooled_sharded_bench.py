#!/usr/bin/env python3
"""Pooled lookups on table-sharded contexts, measured on one MI355X -> profiles/pooled_sharded.json.  Reported, not gating.

Model-C full size, FR_INDEX_PER_TABLE (376 index columns), batch 4096, FR_FILL_HASH, uniform rows, every slot filled.  One child process at a time, each under its own
time limit; the tool stops at the first child that exits abnormally or runs out of time (what was measured until then is written).

  step_hotsN (N = 4, 16): EIGHT shard contexts on the one GPU (the staged exchange: D2H, rendezvous, H2D -- PCIe and host staging, not xGMI), created
      with N slots per column.  Per precision (bf16, fp8; the fp8 exponents from fr_worker_calibrate_fp8_sharded_pooled): the host-clock time of one
      step on all eight ranks (submit on every rank, then every rank's sync) for fr_worker_submit_sharded (one-hot rows) and for
      fr_worker_submit_sharded_pooled on the same contexts and communicators, in alternating blocks of --steps / 2 steps (one-hot, pooled, one-hot,
      pooled; the two forms share the pinned index buffer, which is rewritten before each block, untimed), median over a form's steps, two warm-up steps
      before a form's first block.  And on
      rank 0: the pooled slice gather's kernel time by transport (fr_worker_gather_slices_pooled, fp32 / bf16 / e4m3; HIP events around --reps launches,
      one index buffer).
  reroute: an unsharded context (the slice is the whole record), longest bags of 1 and of 5 slots: the bf16 / e4m3 slice gather, which takes the
      neighbouring shape of gather_pooled_kernel (the two narrow shapes carry no such store), beside the fp32 slice gather through the narrow shape, on
      the same bags: the only evidence on what the re-routing costs (the low-precision forms also store a half / a quarter of the bytes).
  sum points (with --parent-lib PATH, the parent commit's libfleetrec.so): tools/pooled_gather_bench.py --hots 1,4,16 --pool sum (its six padded SUM
      points) with the parent's library and this build's alternating, parent first, twice each.  Per point: the row-rate ratio new / parent (medians
      of the two runs each) and the spread the two parent runs show against each other; "inside" = |ratio - 1| <= that spread.

    python tools/pooled_sharded_bench.py [--parent-lib PATH] [--only step_hots4,reroute,...] [--steps 12] [--reps 200] [--out profiles/pooled_sharded.json]
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SEED_TABLES, SEED_WEIGHTS = 0xF1EE7, 99
G, B = 8, 4096
CHILD_LIMIT_S = 420


def uniform_bags(rng, ranges, hots, batch):
    return (rng.random((batch, len(ranges), hots)) * ranges[None, :, None]).astype(np.int32).reshape(batch, len(ranges) * hots)


def events_us(wk, launch, reps):
    for _ in range(8):
        launch()
    wk.sync()
    wk.timer_start()
    for _ in range(reps):
        launch()
    ms = wk.timer_stop_ms()
    wk.sync()
    return ms * 1e3 / reps


def child_step(fr, hots, steps, reps):
    model = fr.Model.builtin(fr.MODEL_C).clone(index_mode=fr.INDEX_PER_TABLE)
    C = model.idx_cols
    ranges = model.index_ranges()
    rng = np.random.default_rng(880 + hots)
    ctxs, wks = [], []
    for r in range(G):
        c = fr.Context(model, device=0, shard_rank=r, n_shards=G, hots=np.full(C, hots, np.int32))
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        ctxs.append(c)
        wks.append(fr.Worker(c, B))
    comms = fr.Comm.init_all(ctxs)
    ids = uniform_bags(rng, ranges, 1, B)
    bags = uniform_bags(rng, ranges, hots, B)
    dense = rng.uniform(-1, 1, (B, model.dense_len)).astype(np.float32)
    out = {"hots": hots, "ranks": G, "batch": B, "index_cols": int(C), "exchange": "staged host exchange on one GPU", "precisions": {}}

    def all_ranks(fn):
        th = [threading.Thread(target=fn, args=(r,)) for r in range(G)]
        [t.start() for t in th]
        [t.join() for t in th]

    def one_step(pooled):
        t0 = time.perf_counter()
        for r in range(G):
            if pooled:
                wks[r].submit_sharded_pooled(comms[r], B)
            else:
                wks[r].submit_sharded(comms[r], B)
        for r in range(G):
            wks[r].sync()
        return (time.perf_counter() - t0) * 1e3

    for prec, P in (("bf16", fr.FC_BF16), ("fp8", fr.FC_FP8)):
        for c in ctxs:
            c.set_fc_precision(P)
        if prec == "fp8":
            all_ranks(lambda r: wks[r].calibrate_fp8_sharded_pooled(comms[r], bags, dense))
        times = {False: [], True: []}
        for block in range(4):                    # one-hot, pooled, one-hot, pooled: the pinned rows are rewritten before a block (not timed)
            pooled = block % 2 == 1
            for w in wks:
                if pooled:
                    w.load_pooled(bags, dense)
                else:
                    w.idx[:B] = ids
                    w.dense[:B] = dense
            if block < 2:
                one_step(pooled), one_step(pooled)
            times[pooled] += [one_step(pooled) for _ in range(max(steps // 2, 1))]
        e = {"one_hot_step_ms": float(np.median(times[False])), "pooled_step_ms": float(np.median(times[True])),
             "one_hot_step_ms_all": [round(t, 3) for t in times[False]], "pooled_step_ms_all": [round(t, 3) for t in times[True]]}
        if prec == "fp8":
            e["act_exp"] = [int(a) for a in ctxs[0].fp8_exponents()[0]]
        out["precisions"][prec] = e
        print("hots %2d %-4s one-hot step %8.3f ms   pooled step %8.3f ms" % (hots, prec, e["one_hot_step_ms"], e["pooled_step_ms"]), flush=True)
    # rank 0: the pooled slice gather by transport
    ctx, wk = ctxs[0], wks[0]
    F = ctx.shard_info()["slice_padded"]
    d_idx = fr.DeviceBuffer.from_numpy(ctx, bags)
    d_dense = fr.DeviceBuffer.from_numpy(ctx, dense)
    d_out = fr.DeviceBuffer(ctx, B * F * 4)
    out["slice_gather_rank0"] = {"slice_padded_floats": int(F)}
    for name, tp in (("fp32", fr.FC_FP32), ("bf16", fr.FC_BF16), ("e4m3", fr.FC_FP8)):
        us = events_us(wk, lambda: wk.gather_slices_pooled(B, d_idx, d_dense, d_out, tp), reps)
        out["slice_gather_rank0"][name] = {"us": round(us, 3), "kernel": wk.last_kernel()}
        print("hots %2d rank 0 slice gather %-5s %8.2f us  %s" % (hots, name, us, wk.last_kernel()), flush=True)
    for w in wks:
        w.close()
    for cm in comms:
        cm.close()
    for c in ctxs:
        c.close()
    return out


def child_reroute(fr, reps):
    model = fr.Model.builtin(fr.MODEL_C).clone(index_mode=fr.INDEX_PER_TABLE)
    C = model.idx_cols
    ranges = model.index_ranges()
    rng = np.random.default_rng(881)
    out = {"context": "unsharded (the slice is the whole record)", "batch": B, "index_cols": int(C), "bags": {}}
    for hots in (1, 5):
        ctx = fr.Context(model, device=0, hots=np.full(C, hots, np.int32))
        ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
        wk = fr.Worker(ctx, B)
        F = ctx.shard_info()["slice_padded"]
        bags = uniform_bags(rng, ranges, hots, B)
        d_idx = fr.DeviceBuffer.from_numpy(ctx, bags)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (B, model.dense_len)).astype(np.float32))
        d_out = fr.DeviceBuffer(ctx, B * F * 4)
        e = {}
        for rnd in range(3):                          # the three transports alternate
            for name, tp in (("fp32", fr.FC_FP32), ("bf16", fr.FC_BF16), ("e4m3", fr.FC_FP8)):
                us = events_us(wk, lambda: wk.gather_slices_pooled(B, d_idx, d_dense, d_out, tp), reps)
                e.setdefault(name, {"us_rounds": [], "kernel": wk.last_kernel()})["us_rounds"].append(round(us, 3))
        for name in e:
            e[name]["us"] = float(np.median(e[name]["us_rounds"]))
        for name in ("bf16", "e4m3"):
            e[name]["time_over_fp32_narrow_shape"] = e[name]["us"] / e["fp32"]["us"]
        out["bags"]["longest_%d" % hots] = e
        print("longest bag %d: " % hots + "  ".join("%s %.2f us %s" % (n, e[n]["us"], e[n]["kernel"]) for n in e), flush=True)
        wk.close()
        ctx.close()
    return out


def run_child(argv, env=None, limit=CHILD_LIMIT_S):
    """-> (ok, stdout).  The child runs in a process group of its own; at its time limit the group is killed."""
    p = subprocess.Popen(argv, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, start_new_session=True)
    try:
        text, _ = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, 9)
        text, _ = p.communicate()
        return False, text.decode(errors="replace") + "\n[time limit of %d s]" % limit
    return p.returncode == 0, text.decode(errors="replace")


def sum_points(parent_lib, tmp_dir):
    """The six padded SUM points with the parent's library and this build's alternating -> (entry or None, ok)."""
    runs = {"parent": [], "new": []}
    for i in range(2):
        for which in ("parent", "new"):
            path = os.path.join(tmp_dir, "sum_%s_%d.json" % (which, i))
            env = dict(os.environ)
            env.pop("FR_LIB", None)
            if which == "parent":
                env["FR_LIB"] = parent_lib
            ok, text = run_child([sys.executable, os.path.join(ROOT, "tools", "pooled_gather_bench.py"), "--hots", "1,4,16", "--pool", "sum", "--reps", "200", "--out", path], env)
            print(text[-1500:], flush=True)
            if not ok:
                return None, False
            runs[which].append(json.load(open(path)))
    points = {}
    for mi, mode in enumerate(runs["new"][0]["modes"]):
        for shape in mode["shapes"]:
            if not shape.startswith("pooled_hots"):
                continue
            rate = lambda which, i: runs[which][i]["modes"][mi]["shapes"][shape]["row_words_fetched_per_s"]
            p, n = [rate("parent", i) for i in range(2)], [rate("new", i) for i in range(2)]
            ratio, spread = float(np.median(n) / np.median(p)), abs(p[0] / p[1] - 1.0)
            points["%s_%s" % (mode["index_mode"], shape)] = {"parent_row_words_per_s": p, "new_row_words_per_s": n, "row_rate_new_over_parent": ratio,
                                                           "parent_run_to_run_spread": spread, "inside": bool(abs(ratio - 1.0) <= spread)}
    return {"order": "parent, new, parent, new: a fresh process each", "points": points}, True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default="")
    ap.add_argument("--only", default="step_hots4,step_hots16,reroute,sum_points")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooled_sharded.json"))
    args = ap.parse_args()
    if args.child:
        fr = graft.load_package()
        if fr.device_count() < 1:
            sys.exit("pooled_sharded_bench: no MI355X visible")
        res = child_reroute(fr, args.reps) if args.child == "reroute" else child_step(fr, int(args.child[len("step_hots"):]), args.steps, args.reps)
        print("__RESULT__ " + json.dumps(res), flush=True)
        return
    t_start = time.time()
    res = {"tool": "tools/pooled_sharded_bench.py", "model": "C (full size, FR_INDEX_PER_TABLE)", "fill": "FR_FILL_HASH", "index_law": "uniform rows, every slot filled",
           "step_timing": "host clock around submit on all ranks + every rank's sync; median of %d steps per form, in alternating blocks, after 2 warm-up steps" % args.steps,
           "kernel_timing": "HIP events on the worker's stream around %d launches, one index buffer" % args.reps, "not_measured": []}
    wanted = [w for w in args.only.split(",") if w]
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    stopped = False
    for name in wanted:
        if stopped:
            res["not_measured"].append(name + " (not started: an earlier child ended abnormally)")
            continue
        if name == "sum_points":
            if not args.parent_lib or not os.path.exists(args.parent_lib):
                res["not_measured"].append("sum_points (no --parent-lib given)")
                continue
            entry, ok = sum_points(os.path.abspath(args.parent_lib), out_dir)
            for f in os.listdir(out_dir):
                if f.startswith("sum_parent_") or f.startswith("sum_new_"):
                    os.remove(os.path.join(out_dir, f))
            if ok:
                res["sum_points_against_the_parent_library"] = entry
        else:
            ok, text = run_child([sys.executable, os.path.abspath(__file__), "--child", name, "--steps", str(args.steps), "--reps", str(args.reps)])
            print(text[-3000:], flush=True)
            line = [ln for ln in text.splitlines() if ln.startswith("__RESULT__ ")]
            ok = ok and bool(line)
            if ok:
                res[name] = json.loads(line[-1][len("__RESULT__ "):])
        if not ok:
            res["not_measured"].append(name + " (its child process ended abnormally or ran out of time)")
            stopped = True
        res["wall_s"] = round(time.time() - t_start, 1)
        with open(args.out, "w") as f:   # after every child: a later child's trouble loses nothing
            json.dump(res, f, indent=1)
            f.write("\n")
    print("wrote", args.out)
    sys.exit(1 if stopped else 0)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Segmented top-K ranking on one MI355X -> profiles/rank_topk.json.

  (a) rank     HIP-event time of fr_worker_topk_device alone at (n, segments, k) of (256, 1, 16), (4096, 1, 64), (4096, 64, 8), (16384, 1, 256) and
               (2^20, 1024, 32): `--calls` calls back to back between two events on the worker's stream, `--repeats` windows, microseconds per call.
  (b) routes   Model-A (full size) batch 256, host clock per request, both routes of the feature against what a caller does without it:
                 one   submit_device + topk_device (1 segment, k 16) + sync + D2H of the 16 pairs      vs  submit_device + sync + D2H of 256 scores +
                       numpy argpartition + sort
                 four  4 x push_device into one score buffer + topk_device (8 segments of 128, k 16) + sync + D2H of the 8 x 16 pairs
                                                                                                         vs  4 x push_device + sync + D2H of 1024
                       scores + numpy argpartition + sort per segment
               The "without" side needs nothing of the feature: it runs on the same library.
  (c) bench    python bench.py --gpus 1 --steps 20 --warmup 5 against --parent-lib (through FR_LIB) alternating with the product library, `--bench-runs`
               runs each; criterion of profiles/pooled_modes.json: the new median >= the parent's median - (the parent's max - min).

One GPU process at a time: every leg is a child process under its own time limit and in a process group of its own (killed whole at the limit); the
first child that runs into its limit or exits with a non-zero status ends the tool -- what was measured is written, nothing more is started on the card,
the exit status is non-zero.

    python tools/rank_topk_bench.py [--parent-lib <libfleetrec.so of the parent commit>] [--legs rank,routes,bench] [--out profiles/rank_topk.json]
    --rehearse: the CPU back-end, small shapes, host clock: checks the plumbing (its times are not measurements and say so); no bench leg.
"""
import argparse
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = ((256, 1, 16), (4096, 1, 64), (4096, 64, 8), (16384, 1, 256), (2 ** 20, 1024, 32))


def _fr(args):
    import __graft_entry__ as graft
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("rank_topk_bench: no MI355X visible -- a timing needs the GPU")
    return fr


def leg_rank(args):
    fr = _fr(args)
    device = -1 if args.rehearse else 0
    ctx = fr.Context(fr.Model.builtin(fr.MODEL_A).clone(max_rows=200), device=device)
    wk = fr.Worker(ctx, 16)
    rng = np.random.default_rng(77)
    out = {"leg": "rank", "shapes": []}
    for n, n_seg, k in SHAPES:
        if args.rehearse and n > 16384:
            continue
        d_sc = fr.DeviceBuffer.from_numpy(ctx, rng.standard_normal(n).astype(np.float32))
        d_off = fr.DeviceBuffer.from_numpy(ctx, np.arange(0, n + 1, n // n_seg, dtype=np.int32)) if n_seg > 1 else None
        d_i, d_s = fr.DeviceBuffer(ctx, n_seg * k * 4), fr.DeviceBuffer(ctx, n_seg * k * 4)
        call = lambda: wk.topk_device(n, d_sc, k, d_i, d_s, d_off, n_seg)
        for _ in range(3):
            call()
        wk.sync()
        us = []
        for _ in range(args.repeats):
            wk.timer_start()
            for _ in range(args.calls):
                call()
            ms = wk.timer_stop_ms()
            wk.sync()
            us.append(round(1e3 * ms / args.calls, 3))
        out["shapes"].append({"n": n, "segments": n_seg, "k": k, "us_per_call": us, "median_us": float(np.median(us))})
        for b in (d_sc, d_off, d_i, d_s):
            if b is not None:
                b.free()
    wk.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def _host_topk(scores, off, k):
    res = []
    for s in range(len(off) - 1):
        seg = scores[off[s]:off[s + 1]]
        part = np.argpartition(-seg, k - 1)[:k]
        res.append(part[np.argsort(-seg[part], kind="stable")])
    return res


def leg_routes(args):
    fr = _fr(args)
    device = -1 if args.rehearse else 0
    m = fr.Model.builtin(fr.MODEL_A)
    if args.rehearse:
        m = m.clone(max_rows=2000)
    ctx = fr.Context(m, device=device)
    ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
    B, K, NB = 256, 16, 4
    wk = fr.Worker(ctx, B)
    rng = np.random.default_rng(78)
    ranges = m.index_ranges()
    d_idx = [fr.DeviceBuffer.from_numpy(ctx, (rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32)) for _ in range(NB)]
    d_sc = fr.DeviceBuffer(ctx, NB * B * 4)
    part = lambda i: d_sc.ptr.value + i * B * 4
    off8 = np.arange(0, NB * B + 1, 128, dtype=np.int32)
    d_off8 = fr.DeviceBuffer.from_numpy(ctx, off8)
    d_i, d_s = fr.DeviceBuffer(ctx, 8 * K * 4), fr.DeviceBuffer(ctx, 8 * K * 4)

    def one_with():
        wk.submit_device(B, d_idx[0], None, d_sc)
        wk.topk_device(B, d_sc, K, d_i, d_s)
        wk.sync()
        return d_i.download(np.int32, K), d_s.download(np.float32, K)

    def one_without():
        wk.submit_device(B, d_idx[0], None, d_sc)
        wk.sync()
        return _host_topk(d_sc.download(np.float32, B), [0, B], K)

    def four_with():
        for i in range(NB):
            wk.push_device(B, d_idx[i], None, part(i))
        wk.topk_device(NB * B, d_sc, K, d_i, d_s, d_off8, 8)
        wk.sync()
        return d_i.download(np.int32, 8 * K), d_s.download(np.float32, 8 * K)

    def four_without():
        for i in range(NB):
            wk.push_device(B, d_idx[i], None, part(i))
        wk.sync()
        return _host_topk(d_sc.download(np.float32, NB * B), off8, K)

    out = {"leg": "routes", "model": "A", "batch": B, "k": K, "stream_group": ctx.stream_group(), "routes": {}}
    for name, fn in (("one_with", one_with), ("one_without", one_without), ("four_with", four_with), ("four_without", four_without)):
        for _ in range(20):
            fn()
        us = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            us.append(round(1e6 * (time.perf_counter() - t0) / args.calls, 2))
        out["routes"][name] = {"us_per_request": us, "median_us": float(np.median(us))}
    out["both_sides_rank_alike"] = bool(np.array_equal(one_with()[0], one_without()[0]) and np.array_equal(four_with()[0].reshape(8, K), np.stack(four_without())))
    wk.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def child(cmd, env, limit):
    """One child process in a session of its own.  -> (stdout or None, error text or None); at its time limit the whole process group is killed."""
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True, cwd=ROOT)
    try:
        out, err = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        try:
            os.killpg(p.pid, signal.SIGKILL)
        except ProcessLookupError:
            pass
        p.communicate()
        return None, "time limit of %d s: the process group was killed" % limit
    if p.returncode:
        return None, "exit status %d: %s" % (p.returncode, (err or out)[-400:])
    return out, None


def last_json(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    return json.loads(lines[-1]) if lines else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--legs", default="rank,routes,bench")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_topk.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg == "rank":
        return leg_rank(args)
    if args.leg == "routes":
        return leg_routes(args)
    res = {"tool": "tools/rank_topk_bench.py", "one_gpu_process_at_a_time": True, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "not_measured": {}}
    if os.path.exists(args.out):   # legs measured by an earlier call of the tool stay
        try:
            old = json.load(open(args.out))
            if bool(old.get("rehearsal_on_cpu_not_a_measurement")) == bool(args.rehearse):
                for key in ("rank", "routes", "bench"):
                    if key in old:
                        res[key] = old[key]
        except ValueError:
            pass
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    stopped = None
    for leg in [l for l in args.legs.split(",") if l]:
        if stopped:
            res["not_measured"][leg] = "not started: " + stopped
            continue
        if leg in ("rank", "routes"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(args.calls if not args.rehearse else 3), "--repeats", str(args.repeats)]
            out, err = child(cmd + (["--rehearse"] if args.rehearse else []), env, 300)
            got = last_json(out) if out else None
            if not got:
                stopped = "%s ended with: %s" % (leg, (err or "no result line").splitlines()[0][:200])
                res["not_measured"][leg] = err or "no result line"
                continue
            res[leg] = got
            print(leg, json.dumps(got)[:600], flush=True)
        elif leg == "bench":
            if args.rehearse or not args.parent_lib or not os.path.exists(args.parent_lib):
                res["not_measured"]["bench"] = "a rehearsal" if args.rehearse else "no --parent-lib given (or it does not exist)"
                continue
            runs = {"parent": [], "new": []}
            for r in range(args.bench_runs):
                for side in ("parent", "new"):
                    if stopped:
                        break
                    e = dict(env)
                    if side == "parent":
                        e["FR_LIB"] = os.path.abspath(args.parent_lib)
                    out, err = child([sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5"], e, 400)
                    got = last_json(out) if out else None
                    if not got or got.get("value") is None:
                        stopped = "bench.py (%s, run %d) ended with: %s" % (side, r, (err or "no result line").splitlines()[0][:200])
                        break
                    runs[side].append(got["value"])
                    print("bench", side, got["value"], flush=True)
            entry = {"command": "python bench.py --gpus 1 --steps 20 --warmup 5", "unit": "inferences/s", "runs": runs,
                     "criterion": "median(new) >= median(parent) - (max(parent) - min(parent))"}
            if len(runs["parent"]) == args.bench_runs and len(runs["new"]) == args.bench_runs:
                mp, mn, spread = float(np.median(runs["parent"])), float(np.median(runs["new"])), max(runs["parent"]) - min(runs["parent"])
                entry.update({"median_parent": mp, "median_new": mn, "parent_max_minus_min": spread, "criterion_met": bool(mn >= mp - spread)})
            res["bench"] = entry
    if stopped:
        res["stopped"] = stopped
    if not res["not_measured"]:
        del res["not_measured"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if stopped:
        sys.exit("rank_topk_bench: stopped, nothing started after it -- " + stopped)


if __name__ == "__main__":
    main()

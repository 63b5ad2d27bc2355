#!/usr/bin/env python3
"""Request-form batches on one MI355X -> profiles/request_form.json.

  (a) expand   HIP-event time of fr_worker_expand_requests_device alone: `--calls` calls back to back between two events on the worker's stream,
               `--repeats` windows, microseconds per call, and the bytes the launch moves (request rows + candidate rows + offsets + descriptors
               read, expanded rows written) over that time.  Shapes: Model-A rows (47 columns, the first 20 shared) at batch 256 / 4096 / 16384 with
               16 candidates per request; the same split pooled with 4 slots per column at batch 4096; 64 dense floats at batch 4096.
  (b) submit   Model-A (full size), host clock per block with the pinned buffers already filled: fr_worker_submit_requests + sync (the expansion
               reads the pinned request and candidate rows, the chain reads the expanded device rows) against fr_worker_submit + sync on the same
               block as full rows (the chain reads the pinned full rows), alternating, at batch 256 and 4096; and the bytes a block needs in either
               form.  The scores of the two sides are compared bit for bit.
  (c) bench    python bench.py --gpus 1 --steps 20 --warmup 5 against --parent-lib (through FR_LIB) alternating with the product library, `--bench-runs`
               runs each; criterion of profiles/rank_topk.json: the new median >= the parent's median - (the parent's max - min).

One GPU process at a time: every leg is a child process under its own time limit and in a process group of its own (killed whole at the limit); the
first child that runs into its limit or exits with a non-zero status ends the tool -- what was measured is written, nothing more is started on the
card, the exit status is non-zero.

    python tools/request_form_bench.py [--parent-lib <libfleetrec.so of the parent commit>] [--legs expand,submit,bench] [--out profiles/request_form.json]
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
SHARED = 20   # the first 20 of Model-A's 47 index columns are the request's
PER_REQUEST = 16


def _fr(args):
    import __graft_entry__ as graft
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("request_form_bench: no MI355X visible -- a timing needs the GPU")
    return fr


def leg_expand(args):
    fr = _fr(args)
    device = -1 if args.rehearse else 0
    rng = np.random.default_rng(81)
    out = {"leg": "expand", "shapes": []}
    for which, form, batch in (("A", "one_hot", 256), ("A", "one_hot", 4096), ("A", "one_hot", 16384), ("A", "pooled x4", 4096), ("C", "dense", 4096)):
        if args.rehearse and batch > 4096:
            continue
        m = fr.Model.builtin(fr.MODEL_A if which == "A" else fr.MODEL_C).clone(max_rows=200)
        ctx = fr.Context(m, device=device)
        C = m.idx_cols
        shared = (np.arange(C) < SHARED).astype(np.int32)
        if form.startswith("pooled"):
            ctx.set_pooling(np.full(C, 4, np.int32))
        ctx.set_request_columns(shared, dense_shared=which == "C")
        f = {"one_hot": fr.REQ_ONE_HOT, "pooled x4": fr.REQ_POOLED, "dense": fr.REQ_DENSE}[form]
        rs, rc, W = ctx.request_words(f)
        wk = fr.Worker(ctx, batch)
        n_req = batch // PER_REQUEST
        d_req = fr.DeviceBuffer.from_numpy(ctx, rng.integers(0, 2 ** 31, size=max(n_req * rs, 1), dtype=np.int32))
        d_cand = fr.DeviceBuffer.from_numpy(ctx, rng.integers(0, 2 ** 31, size=batch * rc, dtype=np.int32)) if rc else None
        d_off = fr.DeviceBuffer.from_numpy(ctx, np.arange(0, batch + 1, PER_REQUEST, dtype=np.int32))
        d_out = fr.DeviceBuffer(ctx, batch * W * 4)
        call = lambda: wk.expand_requests_device(batch, n_req, d_req, d_cand, d_out, f, d_off)
        for _ in range(3):
            call()
        wk.sync()
        us = []
        for _ in range(args.repeats):
            if args.rehearse:
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    call()
                wk.sync()
                us.append(round(1e6 * (time.perf_counter() - t0) / args.calls, 3))
                continue
            wk.timer_start()
            for _ in range(args.calls):
                call()
            ms = wk.timer_stop_ms()
            wk.sync()
            us.append(round(1e3 * ms / args.calls, 3))
        moved = 4 * (n_req * rs + batch * rc + n_req + 1 + W + batch * W)
        med = float(np.median(us))
        out["shapes"].append({"model": which, "form": form, "batch": batch, "requests": n_req, "request_words": rs, "candidate_words": rc, "row_words": W,
                              "bytes_moved": moved, "us_per_call": us, "median_us": med, "gb_per_s": round(moved / med / 1e3, 2) if med > 0 else None})
        for b in (d_req, d_cand, d_off, d_out):
            if b is not None:
                b.free()
        wk.close()
        ctx.close()
    print(json.dumps(out), flush=True)


def leg_submit(args):
    fr = _fr(args)
    device = -1 if args.rehearse else 0
    m = fr.Model.builtin(fr.MODEL_A)
    if args.rehearse:
        m = m.clone(max_rows=2000)
    ctx = fr.Context(m, device=device)
    ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
    C = m.idx_cols
    shared = (np.arange(C) < SHARED).astype(np.int32)
    ctx.set_request_columns(shared)
    rs, rc, W = ctx.request_words(fr.REQ_ONE_HOT)
    rng = np.random.default_rng(82)
    ranges = m.index_ranges()
    out = {"leg": "submit", "model": "A", "shared_columns": SHARED, "candidates_per_request": PER_REQUEST, "batches": []}
    for B in (256, 4096):
        n_req = B // PER_REQUEST
        wk = fr.Worker(ctx, B)
        req = (rng.random((n_req, rs)) * ranges[None, :rs]).astype(np.int32)
        cand = (rng.random((B, rc)) * ranges[None, rs:]).astype(np.int32)
        full = np.concatenate([np.repeat(req, PER_REQUEST, axis=0), cand], axis=1)
        b_idx, _, _, b_off = wk.request_buffers()
        b_off[:n_req + 1] = np.arange(0, B + 1, PER_REQUEST, dtype=np.int32)
        b_idx[:req.size] = req.ravel()
        flat = np.ctypeslib.as_array(fr.lib().fr_worker_idx_ptr(wk._h), shape=(B * C,))

        def request_form():
            wk.submit_requests(B, n_req, 0)
            wk.sync()

        def full_rows():
            wk.submit(B)
            wk.sync()

        sides = {"request_form": (request_form, cand.ravel()), "full_rows": (full_rows, full.ravel())}
        scores, us = {}, {k: [] for k in sides}
        for name, (fn, rows) in sides.items():
            flat[:rows.size] = rows
            for _ in range(20):
                fn()
            scores[name] = wk.score[:B].copy().view(np.uint32)
        for _ in range(args.repeats):
            for name, (fn, rows) in sides.items():     # alternating
                flat[:rows.size] = rows
                fn()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                us[name].append(round(1e6 * (time.perf_counter() - t0) / args.calls, 2))
        out["batches"].append({"batch": B, "requests": n_req, "bytes_per_block": {"request_form": 4 * (n_req * rs + B * rc), "full_rows": 4 * B * W},
                               "us_per_block": us, "median_us": {k: float(np.median(v)) for k, v in us.items()},
                               "scores_equal_bit_for_bit": bool(np.array_equal(scores["request_form"], scores["full_rows"]))})
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
    ap.add_argument("--legs", default="expand,submit,bench")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "request_form.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg == "expand":
        return leg_expand(args)
    if args.leg == "submit":
        return leg_submit(args)
    res = {"tool": "tools/request_form_bench.py", "options": {"legs": args.legs, "calls": args.calls, "repeats": args.repeats, "bench_runs": args.bench_runs},
           "one_gpu_process_at_a_time": True, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "not_measured": {}}
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    stopped = None
    for leg in [l for l in args.legs.split(",") if l]:
        if stopped:
            res["not_measured"][leg] = "not started: " + stopped
            continue
        if leg in ("expand", "submit"):
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
        sys.exit("request_form_bench: stopped, nothing started after it -- " + stopped)


if __name__ == "__main__":
    main()

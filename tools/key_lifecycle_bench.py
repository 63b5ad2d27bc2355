#!/usr/bin/env python3
"""The life cycle of a key map on one MI355X -> profiles/key_lifecycle.json.  The method and the two MAPPED configurations are
tools/key_resolve_bench.py's: Model-A batch 256 with every column MAPPED, and Model-C batch 4096 per bank with every column MAPPED (up to --max-keys
keys per bank).  Every map holds every key of its column; medians of --repeats windows after a warm-up; the options are recorded in the file.

  (a) rebuild  fr_ctx_rebuild_key_space of EVERY column (same size under a new seed; to twice the size; back) against the only route without it:
               fr_ctx_set_key_space + fr_ctx_put_keys of every live pair from host arrays (chunks of 2^20 pairs).  Both routes are synchronous host
               calls on the context's set-up stream, so the window is the host clock around the calls of all columns (milliseconds); they alternate
               in one process.  Beside the times: keys, slot bytes, and the bytes of pairs the host route sends.
  (b) resolve  HIP-event time of fr_worker_resolve_keys_device on the same batches (every looked-up key present at first) with 0 % of the keys dead,
               with every second key of every map erased, and after the compacting rebuild; fr_ctx_key_space_stats' occupied / live / probe_sum summed
               over the columns beside each figure, so that chain length and time can be read together.
  (c) erase    HIP-event time of fr_worker_erase_keys against fr_worker_put_keys for the same 65536 keys of the largest map (both idempotent:
               `--calls` calls back to back between two events on the worker's stream).

One GPU process at a time: every configuration is a child process under its own time limit and in a process group of its own (killed whole at the
limit); the first child that runs into its limit or exits with a non-zero status ends the tool -- what was measured is written, nothing more is
started on the card, the exit status is non-zero.

    python tools/key_lifecycle_bench.py [--configs A,C] [--out profiles/key_lifecycle.json]
    --rehearse: the CPU back-end, small shapes, host clock: checks the plumbing (its times are not measurements and say so).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import key_resolve_bench as KR  # noqa: E402

ROTATE = KR.ROTATE
ERASE_KEYS = 1 << 16


def slots_of(n):
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def stats_sum(ctx, C):
    s = np.array([ctx.key_space_stats(c) for c in range(C)], np.int64).sum(axis=0)
    return {"slots": int(s[0]), "occupied": int(s[1]), "live": int(s[2]), "probe_sum": int(s[3]), "mean_probes_of_a_present_key": round(1 + s[3] / max(int(s[1]), 1), 4)}


def leg(args):
    fr = KR._fr(args)
    device = -1 if args.rehearse else 0
    which, batch = args.leg, 256 if args.leg == "A" else 4096
    rng = np.random.default_rng(93)
    m = fr.Model.builtin(fr.MODEL_A if which == "A" else fr.MODEL_C)
    index_mode = fr.INDEX_PER_BANK if which == "C" else None
    if index_mode is not None or args.rehearse:
        m = m.clone(index_mode=index_mode, max_rows=2000 if args.rehearse else 0)
    ctx = fr.Context(m, device=device)      # (the tables stay unfilled: nothing here gathers)
    C, ranges = m.idx_cols, np.asarray(m.index_ranges(), np.int64)
    n_keys = np.minimum(ranges, args.max_keys)
    host = []                               # the host arrays of the host route: (keys, rows) per column
    for c in range(C):
        rows = np.arange(int(n_keys[c]), dtype=np.int64)
        host.append((KR.key_of(rows, c), (rows % max(int(ranges[c]) - 1, 1) + 1).astype(np.int32)))   # never row 0, the miss_row

    def host_route(seed, factor=1):
        for c in range(C):
            ctx.set_key_space(c, fr.KEYS_MAPPED, seed=seed + c, max_keys=factor * int(n_keys[c]), miss_row=0)
            k, r = host[c]
            for r0 in range(0, k.size, 1 << 20):
                ctx.put_keys(c, k[r0:r0 + (1 << 20)], r[r0:r0 + (1 << 20)])

    def device_route(seed, factor=1):
        for c in range(C):
            ctx.rebuild_key_space(c, seed + c, factor * int(n_keys[c]))

    def ms(fn, *a):
        ctx.synchronize()
        t0 = time.perf_counter()
        fn(*a)
        ctx.synchronize()
        return round(1e3 * (time.perf_counter() - t0), 3)

    out = {"config": which, "model": which, "index_mode": "per bank" if which == "C" else "model's own", "batch": batch, "index_columns": C,
           "keys_in_maps": int(n_keys.sum()), "slot_bytes": int(sum(16 * slots_of(int(n)) for n in n_keys)), "pair_bytes_the_host_route_sends": int(12 * n_keys.sum())}
    # (a)
    host_route(1000)
    device_route(2000)
    t = {"host_set_key_space_plus_put_keys_ms": [], "device_rebuild_same_size_ms": [], "device_rebuild_twice_the_size_ms": [], "device_rebuild_back_to_size_ms": [],
         "host_set_key_space_plus_put_keys_twice_the_size_ms": []}
    for i in range(args.repeats):           # alternating
        t["host_set_key_space_plus_put_keys_ms"].append(ms(host_route, 3000 + 100 * i))
        t["device_rebuild_same_size_ms"].append(ms(device_route, 4000 + 100 * i))
        t["device_rebuild_twice_the_size_ms"].append(ms(device_route, 5000 + 100 * i, 2))
        t["device_rebuild_back_to_size_ms"].append(ms(device_route, 6000 + 100 * i))
        t["host_set_key_space_plus_put_keys_twice_the_size_ms"].append(ms(host_route, 7000 + 100 * i, 2))
        device_route(1000)
    out["rebuild"] = dict(t, median_ms={k: float(np.median(v)) for k, v in t.items()}, clock="host clock around synchronous calls, all columns")
    # (b)
    wk = fr.Worker(ctx, batch)
    d_keys, d_rows = [], []
    for _ in range(ROTATE):
        rows = (rng.random((batch, C)) * n_keys[None, :]).astype(np.int64)
        d_keys.append(fr.DeviceBuffer.from_numpy(ctx, np.stack([KR.key_of(rows[:, c], c) for c in range(C)], axis=1)))
        d_rows.append(fr.DeviceBuffer(ctx, batch * C * 4))
    resolve = lambda i: wk.resolve_keys_device(batch, d_keys[i % ROTATE], d_rows[i % ROTATE])
    out["resolve"] = []
    for state in ("0 % dead", "every second key erased", "after the compacting rebuild"):
        if state == "every second key erased":
            for c in range(C):
                k = host[c][0][::2]
                for r0 in range(0, k.size, 1 << 20):
                    ctx.erase_keys(c, k[r0:r0 + (1 << 20)])
        elif state == "after the compacting rebuild":
            device_route(1000)
        wk.key_misses()
        us = KR.timed(fr, wk, args.calls, args.repeats, args.rehearse, resolve)
        out["resolve"].append(dict(stats_sum(ctx, C), state=state, resolve_us_per_call=us, median_us=float(np.median(us)),
                                   misses_per_lookup=round(wk.key_misses() / ((2 * ROTATE + args.calls * args.repeats) * batch * C), 4)))
    # (c)
    host_route(1000)
    big = int(np.argmax(n_keys))
    n = min(ERASE_KEYS, int(n_keys[big]))
    pick = rng.permutation(int(n_keys[big]))[:n]
    d_k, d_r = fr.DeviceBuffer.from_numpy(ctx, host[big][0][pick]), fr.DeviceBuffer.from_numpy(ctx, host[big][1][pick])
    us_e = KR.timed(fr, wk, args.calls, args.repeats, args.rehearse, lambda i: wk.erase_keys(big, n, d_k))
    live_after_erase = ctx.key_space_stats(big)[2]
    us_p = KR.timed(fr, wk, args.calls, args.repeats, args.rehearse, lambda i: wk.put_keys(big, n, d_k, d_r))
    assert live_after_erase == int(n_keys[big]) - n and ctx.key_space_stats(big)[2] == int(n_keys[big])
    out["erase"] = {"column": big, "keys_in_map": int(n_keys[big]), "keys_per_call": n, "erase_us_per_call": us_e, "put_us_per_call": us_p,
                    "median_us": {"keymap_erase_kernel": float(np.median(us_e)), "key_put_kernel": float(np.median(us_p))}}
    for b in d_keys + d_rows + [d_k, d_r]:
        b.free()
    wk.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--configs", default="A,C")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-keys", type=int, default=1 << 22, help="keys per MAPPED column at most (a column with fewer rows keys every row)")
    ap.add_argument("--limit", type=int, default=420, help="seconds a configuration's child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_lifecycle.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    res = {"tool": "tools/key_lifecycle_bench.py", "options": {"configs": args.configs, "calls": args.calls, "repeats": args.repeats, "max_keys": args.max_keys},
           "one_gpu_process_at_a_time": True, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "configs": [], "not_measured": {}}
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    stopped = None
    for cfg in [c for c in args.configs.split(",") if c]:
        if stopped:
            res["not_measured"][cfg] = "not started: " + stopped
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", cfg, "--calls", str(args.calls if not args.rehearse else 3), "--repeats", str(args.repeats),
               "--max-keys", str(args.max_keys)]
        out, err = KR.child(cmd + (["--rehearse"] if args.rehearse else []), env, args.limit)
        lines = [ln for ln in (out or "").splitlines() if ln.startswith("{")]
        if not lines:
            stopped = "%s ended with: %s" % (cfg, (err or "no result line").splitlines()[0][:200])
            res["not_measured"][cfg] = err or "no result line"
            continue
        res["configs"].append(json.loads(lines[-1]))
        print(cfg, lines[-1][:1200], flush=True)
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
        sys.exit("key_lifecycle_bench: stopped, nothing started after it -- " + stopped)


if __name__ == "__main__":
    main()

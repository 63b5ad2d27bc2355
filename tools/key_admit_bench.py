#!/usr/bin/env python3
"""Row pools on one MI355X -> profiles/key_admit.json.  ONE map of --pool-rows keys at most (4.19 M: 2^23 slots, 128 MiB) on a one-table model, its
pool the rows [0, pool_rows) of the table; the table has --call-keys more rows, which the puts measured beside the admits use (rows chosen by the
host).  HIP-event windows on the worker's stream after a warm-up, medians of --repeats; everything in one process, the legs alternating.

  (a) admit of --call-keys NEW keys with the pool 0 %, 50 % and about 99 % taken WHEN THE CALL ENDS (it starts call_keys / pool_rows = 1.6 % lower), beside
      fr_worker_put_keys of as many new keys with host-chosen rows.  Neither is idempotent, so a window is ONE call; after every window the keys are
      erased again and the map is compacted (fr_ctx_rebuild_key_space keeps the pool), so that every window of a level starts from the same state.
      An admit is three launches (the call's table filled, keyadmit_admit_kernel, keyadmit_settle_kernel), a put one.
  (b) admit of --call-keys LIVE keys (idempotent: --calls calls per window) beside a resolve of the same keys.
  (c) fr_worker_erase_keys of --call-keys live keys on the column with its pool (keyadmit_release_kernel) and without it (keymap_erase_kernel), one call
      per window, the keys given their rows back in between.
  (d) fr_ctx_set_row_pool over the full map: host clock around the synchronous call (memset, mark pass over every slot, wait).

    python tools/key_admit_bench.py [--out profiles/key_admit.json]
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

COL = 0


def leg(args):
    fr = KR._fr(args)
    device = -1 if args.rehearse else 0
    N, n = args.pool_rows, args.call_keys
    m = fr.Model.from_spec({"name": "one_pool", "tables": [{"dim": 8, "rows": N + n}], "fc": [64, 32, 32]})
    ctx = fr.Context(m, device=device)      # (the table stays unfilled: nothing here gathers)
    ctx.set_key_space(COL, fr.KEYS_MAPPED, seed=77, max_keys=N, miss_row=-1)
    ctx.set_row_pool(COL, 0, N)
    wk = fr.Worker(ctx, n)
    serial = [0]

    def new_keys(count):                    # keys nobody has used yet
        rows = np.arange(serial[0], serial[0] + count, dtype=np.int64)
        serial[0] += count
        return KR.key_of(rows, COL)

    def window(fn, calls=1):
        if args.rehearse:
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            wk.sync()
            return round(1e6 * (time.perf_counter() - t0) / calls, 3)
        wk.timer_start()
        for _ in range(calls):
            fn()
        ms = wk.timer_stop_ms()
        wk.sync()
        return round(1e3 * ms / calls, 3)

    d_k, d_r = fr.DeviceBuffer(ctx, n * 8), fr.DeviceBuffer(ctx, n * 4)
    d_put_rows = fr.DeviceBuffer.from_numpy(ctx, (N + np.arange(n)).astype(np.int32))
    out = {"pool_rows": N, "max_keys": N, "slots": 2 * N if N & (N - 1) == 0 else None, "keys_per_call": n, "admit_new": []}
    filled = 0
    seed = [100]

    def compact():
        seed[0] += 1
        ctx.rebuild_key_space(COL, seed[0], N)

    # (a)
    for level in (0.0, 0.5, 0.99):
        start = max(int(level * N) - n, 0)
        while filled < start:
            step = min(1 << 20, start - filled)
            ctx.admit_keys(COL, new_keys(step))
            filled += step
        assert ctx.row_pool(COL)[2] == N - filled
        t_admit, t_put = [], []
        for i in range(args.warmup + args.repeats):
            keys = new_keys(n)
            d_k.upload(keys)
            us = window(lambda: wk.admit_keys(COL, n, d_k, d_r))
            assert ctx.row_pool(COL)[2] == N - filled - n and np.unique(d_r.download(np.int32, n)).size == n
            wk.erase_keys(COL, n, d_k)
            wk.sync()
            compact()
            keys = new_keys(n)
            d_k.upload(keys)
            us_p = window(lambda: wk.put_keys(COL, n, d_k, d_put_rows))
            wk.erase_keys(COL, n, d_k)
            wk.sync()
            compact()
            assert ctx.row_pool(COL)[2] == N - filled and ctx.key_space(COL)[3] == filled
            if i >= args.warmup:
                t_admit.append(us), t_put.append(us_p)
        out["admit_new"].append({"pool_taken_when_the_call_starts": round(filled / N, 4), "pool_taken_when_the_call_ends": round((filled + n) / N, 4), "keys_in_map_at_start": filled,
                                 "admit_us": t_admit, "put_us": t_put, "median_us": {"admit (fill + keyadmit_admit_kernel + keyadmit_settle_kernel)": float(np.median(t_admit)),
                                                                                  "key_put_kernel": float(np.median(t_put))}})
    # (b) live keys: the admit against a resolve of the same keys
    keys = new_keys(n)
    d_k.upload(keys)
    wk.admit_keys(COL, n, d_k, d_r)
    wk.sync()
    rows = d_r.download(np.int32, n)
    filled += n
    d_out = fr.DeviceBuffer(ctx, n * 4)
    us_a = KR.timed(fr, wk, args.calls, args.repeats, args.rehearse, lambda i: wk.admit_keys(COL, n, d_k, d_r))
    us_r = KR.timed(fr, wk, args.calls, args.repeats, args.rehearse, lambda i: wk.resolve_keys_device(n, d_k, d_out))
    assert np.array_equal(d_r.download(np.int32, n), rows) and np.array_equal(d_out.download(np.int32, n), rows) and ctx.row_pool(COL)[2] == N - filled
    out["admit_live"] = {"pool_taken": round(filled / N, 4), "admit_us_per_call": us_a, "resolve_us_per_call": us_r,
                         "median_us": {"admit of live keys": float(np.median(us_a)), "key_resolve_kernel": float(np.median(us_r))}}
    # (c) and (d)
    d_rows = fr.DeviceBuffer.from_numpy(ctx, rows)
    t_rel, t_era, t_set = [], [], []
    for i in range(args.warmup + args.repeats):
        us = window(lambda: wk.erase_keys(COL, n, d_k))                 # the column has its pool: keyadmit_release_kernel
        assert ctx.row_pool(COL)[2] == N - filled + n
        wk.put_keys(COL, n, d_k, d_rows)                                # the same rows back, by hand ...
        wk.sync()
        ctx.set_row_pool(COL, 0, 0)
        us_e = window(lambda: wk.erase_keys(COL, n, d_k))               # no pool: keymap_erase_kernel
        wk.put_keys(COL, n, d_k, d_rows)
        wk.sync()
        ctx.synchronize()
        t0 = time.perf_counter()
        ctx.set_row_pool(COL, 0, N)                                     # ... which the pool learns of here
        ms = 1e3 * (time.perf_counter() - t0)
        assert ctx.row_pool(COL)[2] == N - filled
        if i >= args.warmup:
            t_rel.append(us), t_era.append(us_e), t_set.append(round(ms, 3))
    out["erase"] = {"keys_per_call": n, "release_us": t_rel, "erase_us": t_era, "median_us": {"keyadmit_release_kernel": float(np.median(t_rel)), "keymap_erase_kernel": float(np.median(t_era))}}
    out["set_row_pool"] = {"slots_walked": ctx.key_space_stats(COL)[0], "live_keys": filled, "ms": t_set, "median_ms": float(np.median(t_set)),
                           "clock": "host clock around the synchronous call"}
    for b in (d_k, d_r, d_put_rows, d_out, d_rows):
        b.free()
    wk.close()
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pool-rows", type=int, default=1 << 22)
    ap.add_argument("--call-keys", type=int, default=1 << 16)
    ap.add_argument("--limit", type=int, default=420, help="seconds the measuring child process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_admit.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.rehearse:
        args.pool_rows, args.call_keys, args.calls = min(args.pool_rows, 1 << 14), min(args.call_keys, 1 << 8), 3
    if args.leg:
        return leg(args)
    res = {"tool": "tools/key_admit_bench.py", "options": {"calls": args.calls, "repeats": args.repeats, "warmup": args.warmup, "pool_rows": args.pool_rows, "call_keys": args.call_keys},
           "one_gpu_process_at_a_time": True, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse)}
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "all", "--calls", str(args.calls), "--repeats", str(args.repeats), "--warmup", str(args.warmup),
           "--pool-rows", str(args.pool_rows), "--call-keys", str(args.call_keys)]
    out, err = KR.child(cmd + (["--rehearse"] if args.rehearse else []), env, args.limit)
    lines = [ln for ln in (out or "").splitlines() if ln.startswith("{")]
    if lines:
        res["result"] = json.loads(lines[-1])
        print(lines[-1][:2000], flush=True)
    else:
        res["stopped"] = err or "no result line"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if not lines:
        sys.exit("key_admit_bench: stopped -- " + res["stopped"])


if __name__ == "__main__":
    main()

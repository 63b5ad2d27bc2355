#!/usr/bin/env python3
"""How long the native driver loop takes for runs of a few batches up to a steady-state run, in one process on one MI355X -> one JSON file.

Workload: the benchmark's headline -- Model-A full size, batch 256, fp32, 2 threads x 2 workers, 1024 rotating index buffers.  For every
`total` in --totals: --warm warm-up calls, then --reps timed calls of Driver.run_resident(256, total, pool) followed by ctx.synchronize();
per call two figures, each reported as median / min / max over the repeats:
  native_us   the `elapsed_s` the C call returns (drain, threads, pushes, launches, syncs, drain: no marshalling of the pool);
  wall_us     the host clock round the Python call plus ctx.synchronize() (what bench.py's timed region sees).
Only entry points every earlier build of ABI 6 has are used, so the same file measures an older tree when it is copied there: it loads the
package next to it (or the build FR_LIB names; the experiments build reads its FR_* knobs, which the file records).

    python tools/driver_burst_probe.py [--out build/driver_burst_probe.json] [--totals 1,5,20,...] [--reps 50] [--warm 5]
    --rehearse: row-capped tables on the CPU back-end, 3 repeats: the plumbing only (its times are not measurements and the file says so).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

SEED_TABLES, SEED_IDX, SEED_WEIGHTS = 0xF1EE7, 1234, 99
B, THREADS, DEPTH, N_POOL = 256, 2, 2, 1024
TOTALS = "1,5,20,63,64,65,129,257,403,20000"


def summary(us):
    return {"median": statistics.median(us), "min": min(us), "max": max(us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "driver_burst_probe.json"))
    ap.add_argument("--totals", default=TOTALS)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warm", type=int, default=5)
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    fr = graft.load_package()
    model = fr.Model.builtin(fr.MODEL_A)
    if args.rehearse:
        model, args.reps, args.warm = model.clone(max_rows=2000), 3, 1
    ctx = fr.Context(model, device=fr.DEVICE_CPU if args.rehearse else 0)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    rng = np.random.default_rng(SEED_IDX)
    n_pool = 16 if args.rehearse else N_POOL
    pool = [fr.DeviceBuffer.from_numpy(ctx, (rng.random((B, model.n_tables)) * model.rows()[None, :]).astype(np.int32)) for _ in range(n_pool)]
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    totals = [int(t) for t in args.totals.split(",")]
    if args.rehearse:
        totals = [t for t in totals if t <= 64]
    else:   # the shader clock ramps over many milliseconds of load: the same >= 0.5 s of work bench.py puts ahead of its timed region
        warm_s = 0.0
        while warm_s < 0.5:
            warm_s += drv.run_resident(B, 8192, pool)
    rows = {}
    for total in totals:
        for _ in range(args.warm):
            drv.run_resident(B, total, pool)
        ctx.synchronize()
        native, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            el = drv.run_resident(B, total, pool)
            ctx.synchronize()
            wall.append(1e6 * (time.perf_counter() - t0))
            native.append(1e6 * el)
        rows[str(total)] = {"native_us": summary(native), "wall_us": summary(wall),
                            "inferences_per_s_wall_median": total * B / (statistics.median(wall) * 1e-6)}
        sys.stderr.write("total %6d: native %9.1f us (%.1f .. %.1f), wall %9.1f us (%.1f .. %.1f)\n" % (
            total, rows[str(total)]["native_us"]["median"], min(native), max(native), rows[str(total)]["wall_us"]["median"], min(wall), max(wall)))
    drv.close()
    out = {"what": "Driver.run_resident(256, total, pool) + ctx.synchronize(): Model-A batch 256 fp32, %d threads x %d workers, %d rotating index buffers, "
                   "%d batches per launch; %d repeats after %d warm-up calls per total, microseconds" % (THREADS, DEPTH, n_pool, ctx.stream_group(), args.reps, args.warm),
           "measured": not args.rehearse, "library": os.path.basename(fr.LIB_PATH),
           "knobs": {k: v for k, v in os.environ.items() if k.startswith("FR_") and k != "FR_LIB"}, "totals": rows}
    if args.rehearse:
        out["what"] = "REHEARSAL on the CPU back-end (not measurements): " + out["what"]
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"out": args.out, "median_wall_us": {k: round(v["wall_us"]["median"], 1) for k, v in rows.items()}}))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Top-K inner-product retrieval on one MI355X -> profiles/retrieve.json.

One table of `--rows` (4 M) rows at dim 32 and one at dim 128, hash-filled; n_q in {1, 32, 256} x k in {16, 256}:
  call_us      HIP-event time of fr_worker_retrieve_device (scan + ranking of the per-chunk lists + row mapping: all its launches), `--calls` calls
               back to back between two events on the worker's stream, `--repeats` windows, the median.
  hbm_share    one pass over the window (rows x dim x 4 bytes) at 8 TB/s over call_us: the floor while n_q <= 32.
  mfma_share   2 x n_q x rows x dim flops at the f32 matrix peak (157.3 TFLOP/s) over call_us: the floor at n_q = 256.
  torch_us     what a caller does today, same shapes, uniform rows of its own: torch.topk(q @ T[chunk].T) over chunks of 2^18 rows, then a final topk
               over the chunks' leaders; torch events.  Measured FIRST, in a child process of its own (torch brings its own HIP runtime, and two
               runtimes do not share a process); a child that ends in anything but a clean exit or a Python error ends the tool.
  adversarial  dim 32, n_q 32, k 256 over rows whose scores ascend with the row for every query: every tile beats every threshold.
The process is the only one on the GPU; a failure ends it with a non-zero status and nothing more is started.

    python tools/retrieve_bench.py [--out profiles/retrieve.json]      --rehearse: the CPU back-end, 20000 rows, no torch leg (times are not measurements)

--image bf16 -> profiles/retrieve_lp.json: the same grid plus dim 16, fr_worker_retrieve_device and fr_worker_retrieve_image_device of the same build
alternating window by window in one process (fp32_us, image_us; speedup = fp32_us / image_us).  Per case the two floors of the image call -- one pass
over the image bytes (rows rounded up to 32 x ceil(dim / 16) x 32 bytes) at 8 TB/s, and 2 x n_q x rows x 16 ceil(dim / 16) flops at the bf16 matrix peak
(2516.8 TFLOP/s) -- with `bound` naming the larger and `share` = that floor over image_us.  Apart: image_build_ms (fr_ctx_set_retrieve_image over the
whole table, host clock around the synchronous call) and fr_worker_update_rows of 1 000 / 100 000 ids without and with an image (the patch is a second
launch: update_ratio = with / without).
--image bf16 --parent-lib <libfleetrec.so of the parent commit, its companions beside it> [--rounds 3]: first, `parent_check`: the fp32 call and an
fr_worker_update_rows without an image on the parent's build (loaded through FR_LIB) and on this one, each run a process of its own, alternating
(parent, this, parent, this, ...); per case the ratio of the medians and the parent's own spread over its runs ((max - min) / median).

--probed -> profiles/retrieve_probed.json: the probed (IVF) retrieval.  4 M hash-filled rows at dim 32 / 128 in equal lists, n_lists in {1024, 4096}, the
centroids a second hash-filled table (recall is not the library's claim and is not measured); n_q in {1, 32, 256} x (n_probe, k) in {(8, 16), (32, 16),
(32, 256)}.  Four legs alternate window by window in one process: coarse_us (fr_worker_retrieve_device over the centroids with k = n_probe), probed_us
(fr_worker_retrieve_probed_device over its output), sum_us (both, back to back, as the composition runs them) and brute_us (fr_worker_retrieve_device over
the whole table: the baseline).  covered_bytes = the bytes of the distinct lists the call's queries probed; covered_hbm_share = those bytes at 8 TB/s over
probed_us; rows_fraction = covered_bytes over the table's.  --parent-lib adds the same parent_check as above.

--filter -> profiles/retrieve_filter.json: the filtered image call (fr_worker_retrieve_image_filtered_device) beside the image call of the same build on the
image grid, legs alternating window by window: every row live and no exclusions, every other tile dead, 64 exclusions per query; the mask's build and
fr_worker_retrieve_filter_rows over 1 000 / 100 000 ids.  --parent-lib: the exact call and the image call (kernels unchanged) against the parent's build.

--probed --image bf16 -> profiles/retrieve_probed_lp.json: the probed retrieval over the table image, the same cells.  Both tables get an image.  The fp32
probed call (probed_fp32_us) and fr_worker_retrieve_probed_image_device (probed_image_us) of the same build alternate window by window in one process,
over the same probe rows (the fp32 coarse call's); speedup = probed_fp32_us / probed_image_us.  Beside them the coarse leg in both forms (coarse_fp32_us,
coarse_image_us), both compositions (sum_fp32_us, sum_image_us) and the brute-force image call (brute_image_us).  covered_image_bytes = the image bytes
of the distinct probed lists (rows x ceil(dim / 16) x 32); covered_hbm_share = those bytes at 8 TB/s over probed_image_us.  --parent-lib: the
parent_check then also times fr_worker_retrieve_probed_device and fr_worker_retrieve_image_device (calls whose kernels did not change) on both builds.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_BYTES_PER_S, MFMA_F32_FLOPS = 8.0e12, 157.3e12


def timed(wk, call, calls, repeats):
    for _ in range(3):
        call()
    wk.sync()
    us = []
    for _ in range(repeats):
        wk.timer_start()
        for _ in range(calls):
            call()
        ms = wk.timer_stop_ms()
        wk.sync()
        us.append(1e3 * ms / calls)
    return float(np.median(us)), [round(u, 2) for u in us]


def torch_route(torch, T, q, k, repeats):
    step = 1 << 18

    def run():
        lead_s, lead_i = [], []
        for a in range(0, T.shape[0], step):
            s, i = torch.topk(q @ T[a:a + step].T, min(k, T[a:a + step].shape[0]), dim=1)
            lead_s.append(s)
            lead_i.append(i + a)
        s, j = torch.topk(torch.cat(lead_s, 1), k, dim=1)
        return torch.gather(torch.cat(lead_i, 1), 1, j), s

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        us.append(1e3 * e0.elapsed_time(e1))
    return float(np.median(us))


def leg_torch(args):
    import torch
    rng, out = np.random.default_rng(91), {}
    for dim in (32, 128):
        T = torch.rand((args.rows, dim), device="cuda") * 2 - 1
        for n_q in (1, 32, 256):
            q = torch.from_numpy(rng.uniform(-1, 1, (n_q, dim)).astype(np.float32)).cuda()
            for k in (16, 256):
                out["%d,%d,%d" % (dim, n_q, k)] = round(torch_route(torch, T, q, k, args.repeats), 2)
        del T
    print(json.dumps(out), flush=True)


MFMA_BF16_FLOPS = 16 * MFMA_F32_FLOPS


def leg_fp32(args, fr):
    """one process: the fp32 call over the grid and the update without an image -> {key: us}"""
    rng, out = np.random.default_rng(91), {}
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": args.rows}, {"dim": 8, "rows": 16}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=-1 if args.rehearse else 0)
        ctx.fill_tables(fr.FILL_HASH, 7)
        wk = fr.Worker(ctx, 16)
        for n in (1000, 100000):
            d_id = fr.DeviceBuffer.from_numpy(ctx, rng.integers(0, args.rows, n).astype(np.int32))
            d_row = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n, dim)).astype(np.float32))
            out["update,%d,%d" % (dim, n)] = round(timed(wk, lambda: wk.update_rows(0, n, d_id, d_row), args.calls, args.repeats)[0], 2)
        for n_q in (1, 32, 256):
            d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
            for k in (16, 256):
                d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
                out["retrieve,%d,%d,%d" % (dim, n_q, k)] = round(timed(wk, lambda: wk.retrieve_device(0, 0, args.rows, n_q, d_q, k, d_r, d_s), args.calls, args.repeats)[0], 2)
        wk.close()
        ctx.close()
    print(json.dumps(out), flush=True)


def leg_unchanged(args, fr):
    """one process: the probed fp32 call and the image call, whose kernels the probed image call left alone, at 4096 lists, n_probe 32, k 16 -> {key: us}"""
    rng, out, n_lists, n_probe, k = np.random.default_rng(91), {}, 4096, 32, 16
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": args.rows}, {"dim": dim, "rows": 4096}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=-1 if args.rehearse else 0)
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_image(0)
        ctx.set_retrieve_lists(0, np.arange(n_lists + 1, dtype=np.int64) * args.rows // n_lists)
        wk = fr.Worker(ctx, 16)
        for n_q in (1, 32, 256):
            d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
            d_p, d_r, d_s = fr.DeviceBuffer(ctx, n_q * n_probe * 4), fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
            wk.retrieve_device(1, 0, n_lists, n_q, d_q, n_probe, d_p, None)
            out["probed,%d,%d" % (dim, n_q)] = round(timed(wk, lambda: wk.retrieve_probed_device(0, n_q, d_q, n_probe, d_p, k, d_r, d_s), args.calls, args.repeats)[0], 2)
            out["image,%d,%d" % (dim, n_q)] = round(timed(wk, lambda: wk.retrieve_image_device(0, 0, args.rows, n_q, d_q, k, d_r, d_s), args.calls, args.repeats)[0], 2)
        wk.close()
        ctx.close()
    print(json.dumps(out), flush=True)


def parent_check(args, leg="fp32"):
    runs = {"parent": [], "this": []}
    for _ in range(args.rounds):
        for setting in ("parent", "this"):
            env = dict(os.environ)
            if setting == "parent":
                env["FR_LIB"] = os.path.abspath(args.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--rows", str(args.rows), "--calls", str(args.calls), "--repeats", str(args.repeats)]
            p = subprocess.run(cmd + (["--rehearse"] if args.rehearse else []), capture_output=True, text=True, timeout=240, env=env)
            if p.returncode != 0:
                sys.exit("retrieve_bench: the %s leg ended with status %d; nothing more is started\n%s" % (setting, p.returncode, p.stderr[-400:]))
            runs[setting].append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    out = []
    for key in runs["this"][0]:
        par, this = [r[key] for r in runs["parent"]], [r[key] for r in runs["this"]]
        out.append({"case": key, "parent_us": par, "this_us": this, "this_over_parent": round(float(np.median(this) / np.median(par)), 4),
                    "parent_spread": round(float((max(par) - min(par)) / np.median(par)), 4)})
        print(json.dumps(out[-1]), flush=True)
    return out


def main_image(args, fr):
    import time
    device, rows = (-1, 20000) if args.rehearse else (0, args.rows)
    res = {"tool": "tools/retrieve_bench.py --image bf16", "rows": rows, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "calls": args.calls,
           "repeats": args.repeats, "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "mfma_bf16_flops": MFMA_BF16_FLOPS}, "cases": [], "image_build": [], "update_rows": []}
    if args.parent_lib:
        res["parent_check"] = parent_check(args)
    rng = np.random.default_rng(91)
    for dim in (16, 32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": rows}, {"dim": 8, "rows": 16}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 7)
        wk = fr.Worker(ctx, 16)
        ups = {}
        for n in (1000, 100000):   # without an image first: the launches of the parent
            ids = rng.integers(0, rows, n).astype(np.int32)
            d_id, d_row = fr.DeviceBuffer.from_numpy(ctx, ids), fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n, dim)).astype(np.float32))
            ups[n] = (d_id, d_row, timed(wk, lambda: wk.update_rows(0, n, d_id, d_row), args.calls, args.repeats)[0])
        builds = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ctx.set_retrieve_image(0)
            builds.append(round(1e3 * (time.perf_counter() - t0), 3))
        steps, tiles = (dim + 15) // 16, (rows + 31) // 32
        image_bytes = tiles * steps * 1024
        res["image_build"].append({"dim": dim, "image_bytes": image_bytes, "table_bytes": rows * dim * 4, "image_build_ms": float(np.median(builds)), "all_ms": builds})
        print(json.dumps(res["image_build"][-1]), flush=True)
        for n, (d_id, d_row, without) in ups.items():
            with_us = timed(wk, lambda: wk.update_rows(0, n, d_id, d_row), args.calls, args.repeats)[0]
            res["update_rows"].append({"dim": dim, "ids": n, "without_image_us": round(without, 2), "with_image_us": round(with_us, 2), "update_ratio": round(with_us / without, 3)})
            print(json.dumps(res["update_rows"][-1]), flush=True)
            d_id.free()
            d_row.free()
        for n_q in (1, 32, 256):
            d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
            for k in (16, 256):
                d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
                calls = {"fp32": lambda: wk.retrieve_device(0, 0, rows, n_q, d_q, k, d_r, d_s), "image": lambda: wk.retrieve_image_device(0, 0, rows, n_q, d_q, k, d_r, d_s)}
                us = {"fp32": [], "image": []}
                for c in calls.values():
                    c()
                wk.sync()
                for _ in range(args.repeats):   # alternating windows
                    for name, c in calls.items():
                        us[name].append(timed(wk, c, args.calls, 1)[0])
                f, i = float(np.median(us["fp32"])), float(np.median(us["image"]))
                hbm_floor, mfma_floor = image_bytes / HBM_BYTES_PER_S, 2.0 * n_q * rows * 16 * steps / MFMA_BF16_FLOPS
                case = {"dim": dim, "n_q": n_q, "k": k, "fp32_us": round(f, 2), "image_us": round(i, 2), "speedup": round(f / i, 3),
                        "fp32_windows_us": [round(u, 2) for u in us["fp32"]], "image_windows_us": [round(u, 2) for u in us["image"]],
                        "bound": "hbm" if hbm_floor >= mfma_floor else "mfma", "share": round(max(hbm_floor, mfma_floor) / (i * 1e-6), 4),
                        "hbm_share": round(hbm_floor / (i * 1e-6), 4), "mfma_share": round(mfma_floor / (i * 1e-6), 4)}
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                d_r.free()
                d_s.free()
            d_q.free()
        wk.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main_probed(args, fr):
    device, rows = (-1, 20000) if args.rehearse else (0, args.rows)
    res = {"tool": "tools/retrieve_bench.py --probed", "rows": rows, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "calls": args.calls,
           "repeats": args.repeats, "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S}, "cases": []}
    if args.parent_lib:
        res["parent_check"] = parent_check(args)
    rng = np.random.default_rng(91)
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": rows}, {"dim": dim, "rows": 4096}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 7)
        wk = fr.Worker(ctx, 16)
        for n_lists in (1024, 4096):
            wk.sync()
            off = np.arange(n_lists + 1, dtype=np.int64) * rows // n_lists
            ctx.set_retrieve_lists(0, off)
            for n_q in (1, 32, 256):
                d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
                for n_probe, k in ((8, 16), (32, 16), (32, 256)):
                    d_p, d_r, d_s = fr.DeviceBuffer(ctx, n_q * n_probe * 4), fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)

                    def coarse():
                        wk.retrieve_device(1, 0, n_lists, n_q, d_q, n_probe, d_p, None)

                    def probed():
                        wk.retrieve_probed_device(0, n_q, d_q, n_probe, d_p, k, d_r, d_s)

                    def both():
                        coarse()
                        probed()

                    calls = {"coarse": coarse, "probed": probed, "sum": both, "brute": lambda: wk.retrieve_device(0, 0, rows, n_q, d_q, k, d_r, d_s)}
                    us = {name: [] for name in calls}
                    both()
                    wk.sync()
                    ids = d_p.download(np.int32, n_q * n_probe)
                    for _ in range(args.repeats):   # alternating windows
                        for name, c in calls.items():
                            us[name].append(timed(wk, c, args.calls, 1)[0])
                    med = {name: float(np.median(v)) for name, v in us.items()}
                    list_bytes = np.diff(off)[ids] * dim * 4   # every pair's list; a list that several queries probe is counted once in covered_bytes
                    covered = int(np.diff(off)[np.unique(ids)].sum() * dim * 4)
                    case = {"dim": dim, "n_lists": n_lists, "n_q": n_q, "n_probe": n_probe, "k": k, "coarse_us": round(med["coarse"], 2), "probed_us": round(med["probed"], 2),
                            "sum_us": round(med["sum"], 2), "brute_us": round(med["brute"], 2), "brute_over_sum": round(med["brute"] / med["sum"], 3),
                            "rows_fraction": round(covered / (rows * dim * 4), 5), "covered_bytes": covered, "pair_bytes": int(list_bytes.sum()),
                            "covered_hbm_share": round(covered / HBM_BYTES_PER_S / (med["probed"] * 1e-6), 4),
                            "windows_us": {name: [round(u, 2) for u in v] for name, v in us.items()}}
                    res["cases"].append(case)
                    print(json.dumps({key: v for key, v in case.items() if key != "windows_us"}), flush=True)
                    for b in (d_p, d_r, d_s):
                        b.free()
                d_q.free()
        wk.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main_probed_image(args, fr):
    device, rows = (-1, 20000) if args.rehearse else (0, args.rows)
    res = {"tool": "tools/retrieve_bench.py --probed --image bf16", "rows": rows, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "calls": args.calls,
           "repeats": args.repeats, "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S}, "cases": []}
    if args.parent_lib:
        res["parent_check"] = parent_check(args, "unchanged")
    rng = np.random.default_rng(91)
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": rows}, {"dim": dim, "rows": 4096}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_image(0)
        ctx.set_retrieve_image(1)
        wk = fr.Worker(ctx, 16)
        row_bytes = 32 * ((dim + 15) // 16)   # of one row in the image
        for n_lists in (1024, 4096):
            wk.sync()
            off = np.arange(n_lists + 1, dtype=np.int64) * rows // n_lists
            ctx.set_retrieve_lists(0, off)
            for n_q in (1, 32, 256):
                d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
                for n_probe, k in ((8, 16), (32, 16), (32, 256)):
                    d_p, d_pi = fr.DeviceBuffer(ctx, n_q * n_probe * 4), fr.DeviceBuffer(ctx, n_q * n_probe * 4)   # d_pi: what the image coarse leg writes, not probed
                    d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
                    calls = {"coarse_fp32": lambda: wk.retrieve_device(1, 0, n_lists, n_q, d_q, n_probe, d_pi, None),
                             "coarse_image": lambda: wk.retrieve_image_device(1, 0, n_lists, n_q, d_q, n_probe, d_pi, None),
                             "probed_fp32": lambda: wk.retrieve_probed_device(0, n_q, d_q, n_probe, d_p, k, d_r, d_s),
                             "probed_image": lambda: wk.retrieve_probed_image_device(0, n_q, d_q, n_probe, d_p, k, d_r, d_s),
                             "brute_image": lambda: wk.retrieve_image_device(0, 0, rows, n_q, d_q, k, d_r, d_s)}
                    calls["sum_fp32"] = lambda: (calls["coarse_fp32"](), calls["probed_fp32"]())
                    calls["sum_image"] = lambda: (calls["coarse_image"](), calls["probed_image"]())
                    wk.retrieve_device(1, 0, n_lists, n_q, d_q, n_probe, d_p, None)   # the probe rows both probed legs scan
                    for c in calls.values():
                        c()
                    wk.sync()
                    ids = d_p.download(np.int32, n_q * n_probe)
                    us = {name: [] for name in calls}
                    for _ in range(args.repeats):   # alternating windows
                        for name, c in calls.items():
                            us[name].append(timed(wk, c, args.calls, 1)[0])
                    med = {name: float(np.median(v)) for name, v in us.items()}
                    covered = int(np.diff(off)[np.unique(ids)].sum() * row_bytes)
                    case = {"dim": dim, "n_lists": n_lists, "n_q": n_q, "n_probe": n_probe, "k": k}
                    case.update({name + "_us": round(v, 2) for name, v in med.items()})
                    case.update({"speedup": round(med["probed_fp32"] / med["probed_image"], 3), "sum_speedup": round(med["sum_fp32"] / med["sum_image"], 3),
                                 "brute_image_over_sum_image": round(med["brute_image"] / med["sum_image"], 3), "covered_image_bytes": covered,
                                 "covered_hbm_share": round(covered / HBM_BYTES_PER_S / (med["probed_image"] * 1e-6), 4),
                                 "windows_us": {name: [round(u, 2) for u in v] for name, v in us.items()}})
                    res["cases"].append(case)
                    print(json.dumps({key: v for key, v in case.items() if key != "windows_us"}), flush=True)
                    for b in (d_p, d_pi, d_r, d_s):
                        b.free()
                d_q.free()
        wk.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def leg_plain(args, fr):
    """one process: the exact call and the image call, whose kernels the filtered call left alone, at k 16 -> {key: us}"""
    rng, out, k = np.random.default_rng(91), {}, 16
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": args.rows}, {"dim": 8, "rows": 16}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=-1 if args.rehearse else 0)
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        for n_q in (1, 32, 256):
            d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
            d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
            out["fp32,%d,%d" % (dim, n_q)] = round(timed(wk, lambda: wk.retrieve_device(0, 0, args.rows, n_q, d_q, k, d_r, d_s), args.calls, args.repeats)[0], 2)
            out["image,%d,%d" % (dim, n_q)] = round(timed(wk, lambda: wk.retrieve_image_device(0, 0, args.rows, n_q, d_q, k, d_r, d_s), args.calls, args.repeats)[0], 2)
        wk.close()
        ctx.close()
    print(json.dumps(out), flush=True)


def main_filter(args, fr):
    """the filtered image call beside the image call of the same build, legs alternating window by window: (a) every row live, no exclusions; (b) every
    other tile of 32 rows dead; (c) 64 exclusions per query (rows drawn from the whole table); the mask's build and its patches of 1 000 / 100 000 ids"""
    import time
    device, rows = (-1, 20000) if args.rehearse else (0, args.rows)
    res = {"tool": "tools/retrieve_bench.py --filter", "rows": rows, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "calls": args.calls,
           "repeats": args.repeats, "cases": [], "mask_build": [], "filter_rows": []}
    if args.parent_lib:
        res["parent_check"] = parent_check(args, "plain")
    rng = np.random.default_rng(91)
    half = (np.arange(rows, dtype=np.int32).reshape(-1, 32)[::2]).reshape(-1) if rows % 64 == 0 else np.arange(0, rows, 2, dtype=np.int32)
    for dim in (16, 32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": rows}, {"dim": 8, "rows": 16}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        builds = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            ctx.set_retrieve_filter(0)
            builds.append(round(1e3 * (time.perf_counter() - t0), 3))
        res["mask_build"].append({"dim": dim, "mask_bytes": (rows + 31) // 32 * 4, "mask_build_ms": float(np.median(builds)), "all_ms": builds})
        print(json.dumps(res["mask_build"][-1]), flush=True)
        if dim == 16:
            for n in (1000, 100000):
                d_id = fr.DeviceBuffer.from_numpy(ctx, rng.integers(0, rows, n).astype(np.int32))
                us = timed(wk, lambda: wk.retrieve_filter_rows(0, n, d_id, True), args.calls, args.repeats)
                res["filter_rows"].append({"ids": n, "us": round(us[0], 2), "windows_us": us[1]})
                print(json.dumps(res["filter_rows"][-1]), flush=True)
                d_id.free()
        d_half = fr.DeviceBuffer.from_numpy(ctx, half)
        for n_q in (1, 32, 256):
            d_q = fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (n_q, dim)).astype(np.float32))
            d_x = fr.DeviceBuffer.from_numpy(ctx, rng.integers(0, rows, (n_q, 64)).astype(np.int32))
            for k in (16, 256):
                d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
                image = lambda: wk.retrieve_image_device(0, 0, rows, n_q, d_q, k, d_r, d_s)
                plain = lambda: wk.retrieve_image_filtered_device(0, 0, rows, n_q, d_q, 0, None, k, d_r, d_s)
                excl = lambda: wk.retrieve_image_filtered_device(0, 0, rows, n_q, d_q, 64, d_x, k, d_r, d_s)
                us = {"image": [], "all_live": [], "excl_64": [], "image_2": [], "half_dead": []}
                for _ in range(args.repeats):   # alternating windows
                    for name, c in (("image", image), ("all_live", plain), ("excl_64", excl)):
                        us[name].append(timed(wk, c, args.calls, 1)[0])
                wk.retrieve_filter_rows(0, len(half), d_half, False)
                for _ in range(args.repeats):
                    for name, c in (("image_2", image), ("half_dead", plain)):
                        us[name].append(timed(wk, c, args.calls, 1)[0])
                wk.retrieve_filter_rows(0, len(half), d_half, True)
                wk.sync()
                med = {name: float(np.median(v)) for name, v in us.items()}
                case = {"dim": dim, "n_q": n_q, "k": k, **{name + "_us": round(v, 2) for name, v in med.items()},
                        "all_live_over_image": round(med["all_live"] / med["image"], 3), "excl_64_over_image": round(med["excl_64"] / med["image"], 3),
                        "half_dead_over_image": round(med["half_dead"] / med["image_2"], 3), "windows_us": {name: [round(u, 2) for u in v] for name, v in us.items()}}
                res["cases"].append(case)
                print(json.dumps({key: v for key, v in case.items() if key != "windows_us"}), flush=True)
                d_r.free()
                d_s.free()
            d_q.free()
            d_x.free()
        d_half.free()
        wk.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filter", action="store_true")
    ap.add_argument("--probed", action="store_true")
    ap.add_argument("--image", default="", choices=("", "bf16"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--leg", default="")
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", "retrieve_filter.json" if args.filter else "retrieve_probed_lp.json" if args.probed and args.image else
                                        "retrieve_probed.json" if args.probed else "retrieve_lp.json" if args.image else "retrieve.json")
    if args.leg == "torch":
        return leg_torch(args)
    if args.filter or args.probed or args.image or args.leg in ("fp32", "unchanged", "plain"):
        import __graft_entry__ as graft
        fr = graft.load_package()
        if not args.rehearse and fr.device_count() < 1:
            sys.exit("retrieve_bench: no MI355X visible -- a timing needs the GPU")
        if args.rehearse:
            args.rows = 20000
        if args.leg:
            return leg_fp32(args, fr) if args.leg == "fp32" else leg_plain(args, fr) if args.leg == "plain" else leg_unchanged(args, fr)
        if args.filter:
            return main_filter(args, fr)
        return main_probed_image(args, fr) if args.probed and args.image else main_probed(args, fr) if args.probed else main_image(args, fr)
    torch_us, torch_note = {}, None
    if not args.rehearse:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "torch", "--rows", str(args.rows), "--repeats", str(args.repeats)],
                               capture_output=True, text=True, timeout=300)
        except subprocess.TimeoutExpired:
            sys.exit("retrieve_bench: the torch leg ran into its time limit; nothing more is started")
        if p.returncode not in (0, 1):
            sys.exit("retrieve_bench: the torch leg ended with status %d; nothing more is started" % p.returncode)
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        if p.returncode == 0 and lines:
            torch_us = json.loads(lines[-1])
        else:
            torch_note = "not measured: " + (p.stderr.strip().splitlines() or ["no result"])[-1][:200]
            print("torch leg", torch_note, flush=True)
    import __graft_entry__ as graft
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("retrieve_bench: no MI355X visible -- a timing needs the GPU")
    device, rows = (-1, 20000) if args.rehearse else (0, args.rows)
    res = {"tool": "tools/retrieve_bench.py", "rows": rows, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "calls": args.calls, "repeats": args.repeats,
           "peaks": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "mfma_f32_flops": MFMA_F32_FLOPS}, "cases": []}
    if torch_note:
        res["torch_us"] = torch_note
    rng = np.random.default_rng(91)
    for dim in (32, 128):
        m = fr.Model.from_spec({"name": "retrieve", "tables": [{"dim": dim, "rows": rows}, {"dim": 8, "rows": 16}], "fc": [32, 32, 32]})
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 7)
        wk = fr.Worker(ctx, 16)
        for n_q in (1, 32, 256):
            Q = rng.uniform(-1, 1, (n_q, dim)).astype(np.float32)
            d_q = fr.DeviceBuffer.from_numpy(ctx, Q)
            for k in (16, 256):
                d_r, d_s = fr.DeviceBuffer(ctx, n_q * k * 4), fr.DeviceBuffer(ctx, n_q * k * 4)
                us, all_us = timed(wk, lambda: wk.retrieve_device(0, 0, rows, n_q, d_q, k, d_r, d_s), args.calls, args.repeats)
                case = {"dim": dim, "n_q": n_q, "k": k, "call_us": round(us, 2), "windows_us": all_us,
                        "hbm_share": round(rows * dim * 4 / HBM_BYTES_PER_S / (us * 1e-6), 4), "mfma_share": round(2.0 * n_q * rows * dim / MFMA_F32_FLOPS / (us * 1e-6), 4)}
                if "%d,%d,%d" % (dim, n_q, k) in torch_us:
                    case["torch_us"] = torch_us["%d,%d,%d" % (dim, n_q, k)]
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                d_r.free()
                d_s.free()
            d_q.free()
        if dim == 32:   # every query's score ascends with the row
            step = 1 << 18
            for a in range(0, rows, step):
                part = np.zeros((min(step, rows - a), dim), np.float32)
                part[:, 0] = np.arange(a, a + len(part))
                ctx.upload_table(0, part, row0=a)
            Q = np.zeros((32, dim), np.float32)
            Q[:, 0] = 1
            d_q, d_r, d_s = fr.DeviceBuffer.from_numpy(ctx, Q), fr.DeviceBuffer(ctx, 32 * 256 * 4), fr.DeviceBuffer(ctx, 32 * 256 * 4)
            us, all_us = timed(wk, lambda: wk.retrieve_device(0, 0, rows, 32, d_q, 256, d_r, d_s), args.calls, args.repeats)
            top = d_r.download(np.int32, 32 * 256).reshape(32, 256)
            res["adversarial"] = {"dim": dim, "n_q": 32, "k": 256, "call_us": round(us, 2), "windows_us": all_us,
                                  "last_rows_first": bool((top == np.arange(rows - 1, rows - 257, -1)[None, :]).all())}
            print(json.dumps(res["adversarial"]), flush=True)
            for b in (d_q, d_r, d_s):
                b.free()
        wk.close()
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Pooled lookups end to end, three ways, on one MI355X -> profiles/pooled_stream.json.

  (a) submit   fr_worker_submit_pooled_device + fr_worker_sync per batch: the only pooled path before the streaming pushes.  Timed on the build
               named by --parent-lib (the commit before them), in the same session; "not measured" without one.
  (b) push     fr_worker_push_pooled_device_list: the pooled gather stores the chain's stage-1 operand itself, the stage pipeline stays in flight.
  (b_exp)      form (b) on the experiments build with the knob off: that build reads its knobs from the environment at every call, a host cost
               per push that (c) pays too -- c / b_exp is the two-launch form's own price.
  (c) two      the same pushes with the gather writing fp32 records and the conversion launch of fr_worker_fc_only behind it: the experiments
               build (libfleetrec_exp.so) with FR_POOL_PUSH_TWO_LAUNCH=1.  The product library reads no environment variable.

Configurations: Model-A batch 256 fp32; Model-C batch 4096 FR_INDEX_PER_BANK bf16 and fp8; each at hots 4 and 16 on every column, every slot
filled, uniform rows, FR_FILL_HASH tables, 8 rotating index buffers.  One GPU process at a time: every (configuration, form) is a child process
under its own time limit and in a process group of its own (killed whole at the limit); the first child that runs into its limit or exits with
a non-zero status ends the tool -- what was measured is written, nothing more is started on the card, the exit status is non-zero.  A child warms up
both hots, then times `--repeats` windows of at least `--seconds` of steady state each (host clock around a window that ends in fr_worker_sync) and
prints inferences/s per window.  The gather kernel's own time in (b) and (c) comes from
`rocprofv3 --kernel-trace --stats` runs of their own (short windows; tracing slows the host, so no rate is taken from them).

Per configuration and hots the file holds the three forms' windows, their medians, the spread (max - min of a form's windows, the largest of the
three forms), and the two acceptance readings: (b) not below (a) by more than the spread; (c) above (b) by more than the spread or not.

    python tools/pooled_stream_bench.py --parent-lib <libfleetrec.so of the parent commit> [--out profiles/pooled_stream.json] [--seconds 2] [--repeats 3]
    --rehearse: tiny tables on the CPU back-end, short windows, no profiler: checks the plumbing (its rates are not measurements and say so).
"""
import argparse
import csv
import glob
import json
import os
import signal
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd")
CONFIGS = {"A256_fp32": ("A", 256, "fp32"), "C4096_bank_bf16": ("C", 4096, "bf16"), "C4096_bank_fp8": ("C", 4096, "fp8")}
HOTS = (4, 16)
NBUF, LIST = 8, 64


def leg(args):
    """One (configuration, form) in this process: JSON on the last line of stdout."""
    import __graft_entry__ as graft
    fr = graft.load_package()
    which, B, prec = CONFIGS[args.config]
    device = -1 if args.rehearse else 0
    if args.rehearse:
        B = min(B, 32)   # (the CPU back-end: plumbing only)
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("pooled_stream_bench: no MI355X visible -- a timing needs the GPU")
    model = fr.Model.builtin(fr.MODEL_A if which == "A" else fr.MODEL_C)
    kw = {"index_mode": fr.INDEX_PER_BANK} if which == "C" else {}
    if args.rehearse:
        kw["max_rows"] = 2000
    model = model.clone(**kw) if kw else model
    ctx = fr.Context(model, device=device)
    ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
    if prec != "fp32" and not args.rehearse:
        ctx.set_fc_precision(fr.FC_BF16 if prec == "bf16" else fr.FC_FP8)
    rng = np.random.default_rng(4242)
    ranges = model.index_ranges()
    out = {"config": args.config, "form": args.form, "library": os.environ.get("FR_LIB", "libfleetrec.so"), "hots": {}}
    for h in HOTS:
        ctx.set_pooling(np.full(model.idx_cols, h, np.int32))
        wk = fr.Worker(ctx, B)
        idx = [fr.DeviceBuffer.from_numpy(ctx, (rng.random((B, len(ranges), h)) * ranges[None, :, None]).astype(np.int32).reshape(B, -1)) for _ in range(NBUF)]
        dense = [fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (B, model.dense_len)).astype(np.float32)) for _ in range(NBUF)] if model.dense_len else None
        scores = [fr.DeviceBuffer(ctx, B * 4) for _ in range(NBUF)]
        if args.form == "submit":
            def run(n):
                for i in range(n):
                    k = i % NBUF
                    wk.submit_pooled_device(B, idx[k], dense[k] if dense else None, scores[k])
                    wk.sync()
        else:
            ks = [i % NBUF for i in range(LIST)]
            plist = wk.make_pooled_push_list([B] * LIST, [idx[k] for k in ks], [dense[k] for k in ks] if dense else None, [scores[k] for k in ks])

            def run(n):
                for _ in range(max(1, n // LIST)):
                    wk.push_pooled_device_list(plist)
                wk.sync()
        run(2 * LIST)   # warm-up: code objects, the tables' first touch, the chain width
        kernel = wk.last_kernel()
        t0 = time.perf_counter()
        run(4 * LIST)
        per = (time.perf_counter() - t0) / (4 * LIST)
        n = max(LIST, int(args.seconds / per) // LIST * LIST)
        rates = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            run(n)
            rates.append(n * B / (time.perf_counter() - t0))
        out["hots"][str(h)] = {"gather_kernel": kernel, "batches_per_window": n, "inferences_per_s": [round(r) for r in rates]}
        wk.close()
        for b in idx + scores + (dense or []):
            b.free()
        ctx.set_pooling(None)
    ctx.close()
    print(json.dumps(out), flush=True)


def child(args, config, form, lib, seconds, repeats, profile_dir=None, limit=240):
    """One leg as a child process in a session of its own.  -> (result or None, error text or None).  A child that runs into its time limit has its
    whole process group killed (under the profiler the process that holds the GPU is a grandchild); that, or any non-zero exit status, is an
    error the caller must stop at: nothing more is started on a card after a program on it hung, faulted or aborted."""
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    env.pop("FR_POOL_PUSH_TWO_LAUNCH", None)
    if lib:
        env["FR_LIB"] = lib
    if form == "two":
        env["FR_POOL_PUSH_TWO_LAUNCH"] = "1"
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--config", config, "--form", "push" if form == "two" else form, "--seconds", str(seconds),
           "--repeats", str(repeats)] + (["--rehearse"] if args.rehearse else [])
    if profile_dir:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", profile_dir, "--output-format", "csv", "--"] + cmd
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, start_new_session=True)
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
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    if not lines:
        return None, "no result line"
    return json.loads(lines[-1]), None


def gather_kernel_us(profile_dir):
    """-> {kernel name: average microseconds} of the gather_pooled_kernel rows in rocprofv3's kernel statistics."""
    res = {}
    for path in glob.glob(os.path.join(profile_dir, "**", "*kernel_stats.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if "gather_pooled_kernel" in name or "records_to_q" in name or "transpose_records_kernel" in name:
                    short = name.split("(")[0].replace("void ", "")
                    res[short] = {"calls": int(row.get("Calls", 0)), "average_us": round(float(row.get("AverageNs", 0)) / 1e3, 3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--config", default="")
    ap.add_argument("--form", default="push")
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--exp-lib", default=os.path.join(PKG, "libfleetrec_exp.so"))
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooled_stream.json"))
    ap.add_argument("--profile-dir", default="")
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    seconds = 0.05 if args.rehearse else args.seconds
    res = {"tool": "tools/pooled_stream_bench.py", "fill": "FR_FILL_HASH", "index_law": "uniform rows, every slot filled", "index_buffers": NBUF,
           "batches_per_list_call": LIST, "seconds_per_window_at_least": seconds, "windows_per_form": args.repeats,
           "timing": "host clock around a window that ends in fr_worker_sync; one GPU process at a time, one child process per (configuration, form)",
           "forms": {"a": "submit_pooled_device + sync per batch, parent build", "b": "push_pooled_device_list, product build",
                     "b_exp": "the same on the experiments build, knob off (that build reads its knobs from the environment at every call: c / b_exp is free of it)",
                     "c": "the same pushes, gather to records + conversion launch (experiments build, FR_POOL_PUSH_TWO_LAUNCH=1)"},
           "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "configs": {}}
    # b_exp: form (b) on the experiments build with the knob off -- that build reads its knobs from the environment at every call, a host cost per push
    # that form (c) pays too: c / b_exp is the two-launch form's own price, c / b also carries the build's
    libs = {"a": ("submit", args.parent_lib or None), "b": ("push", None), "b_exp": ("push", args.exp_lib), "c": ("two", args.exp_lib)}
    stopped = None   # the first child that hung or ended abnormally: nothing is started after it
    for config in [c for c in args.configs.split(",") if c]:
        entry = {"hots": {str(h): {} for h in HOTS}, "not_measured": {}}
        for tag, (form, lib) in libs.items():
            if stopped:
                entry["not_measured"][tag] = "not started: " + stopped
                continue
            if tag == "a" and not lib and not args.rehearse:
                entry["not_measured"][tag] = "no --parent-lib given"
                continue
            if lib and not os.path.exists(lib):
                entry["not_measured"][tag] = "%s not built" % os.path.basename(lib)
                continue
            if args.rehearse and tag in ("b_exp", "c"):
                entry["not_measured"][tag] = "the knob needs the experiments build on a GPU"
                continue
            got, err = child(args, config, form, lib, seconds, args.repeats)
            if not got:
                stopped = "%s (%s) ended with: %s" % (config, tag, err.splitlines()[0][:160])
                entry["not_measured"][tag] = err
                continue
            for h, e in got["hots"].items():
                entry["hots"][h][tag] = e
            print(config, tag, {h: e["inferences_per_s"] for h, e in got["hots"].items()}, flush=True)
        for h, forms in entry["hots"].items():
            med = {t: float(np.median(e["inferences_per_s"])) for t, e in forms.items()}
            spread = max([max(e["inferences_per_s"]) - min(e["inferences_per_s"]) for e in forms.values()] or [0])
            forms["median_inferences_per_s"] = {t: round(v) for t, v in med.items()}
            forms["spread_inferences_per_s"] = spread
            if "a" in med and "b" in med:
                forms["b_not_below_a_by_more_than_the_spread"] = bool(med["b"] >= med["a"] - spread)
                forms["b_over_a"] = round(med["b"] / med["a"], 3)
            if "b" in med and "c" in med:
                forms["c_beats_b_by_more_than_the_spread"] = bool(med["c"] > med["b"] + spread)
                forms["c_over_b"] = round(med["c"] / med["b"], 3)
            if "b_exp" in med and "c" in med:
                forms["c_beats_b_exp_by_more_than_the_spread"] = bool(med["c"] > med["b_exp"] + spread)
                forms["c_over_b_exp"] = round(med["c"] / med["b_exp"], 3)
        if args.profile_dir and not args.rehearse:   # the gather kernel's own time, in runs of their own
            entry["gather_kernel_us"] = {}
            for tag in ("b", "c"):
                form, lib = libs[tag]
                if lib and not os.path.exists(lib):
                    continue
                if stopped:
                    entry["gather_kernel_us"][tag] = {"not_measured": "not started: " + stopped}
                    continue
                pdir = os.path.join(args.profile_dir, "%s_%s" % (config, tag))
                got, err = child(args, config, form, lib, 0.2, 1, profile_dir=pdir, limit=300)
                if not got:
                    stopped = "%s (%s, profiler run) ended with: %s" % (config, tag, err.splitlines()[0][:160])
                entry["gather_kernel_us"][tag] = gather_kernel_us(pdir) if got else {"not_measured": err}
        if not entry["not_measured"]:
            del entry["not_measured"]
        res["configs"][config] = entry
    if stopped:
        res["stopped"] = stopped
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if stopped:
        sys.exit("pooled_stream_bench: stopped, nothing started after it -- " + stopped)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What the per-layer epilogue (fr_ctx_set_epilogue: bias + ReLU) costs, on one MI355X -> profiles/fc_epilogue.json (key "epilogue_cost").

Shapes: Model-A batch 256 fp32 at stream group 64 (the 64-item kernel) and at stream group 16 (the 32-item kernel: with an epilogue its sibling
<2, 44, 2, true>, one workgroup per CU), Model-B batch 1024 bf16 (stream group 128: with an epilogue the chunked kernel for the persistent one),
Model-C batch 4096 FR_INDEX_PER_BANK bf16 and fp8 (stage pipeline + GEMM launches, pushes of one batch).  For each: steady-state inferences/s of fr_worker_push_device_list with no epilogue and with
a bias on all four layers + ReLU on the three hidden ones, the ratio of the medians, and the kernel each run reported (fr_worker_last_kernel) -- so a
shape whose epilogue context takes a sibling kernel shows what that costs.  FR_FILL_HASH tables, FR_WEIGHTS_UNIFORM, uniform
float biases, 8 rotating index buffers; fp8 is calibrated per setting.  One GPU process at a time: every (shape, setting) is a child process under its
own time limit, in a process group of its own (killed whole at the limit); the first child that runs into its limit or exits with a non-zero status
ends the tool -- what was measured is written, nothing more is started on the card, the exit status is non-zero.

--parent-lib <libfleetrec.so of the parent commit, its companions beside it>: a third setting per shape, "parent" = no epilogue on that build (loaded
through FR_LIB) in the same session, and the ratio none / parent: the default path against the commit before the epilogue.
--rounds R: the settings of a shape are run R times in alternation (parent, none, epilogue, parent, none, ...), each run a process of its own; a
setting's windows are those of all its runs.

    python tools/fc_epilogue_bench.py [--parent-lib PATH] [--out profiles/fc_epilogue.json] [--seconds 2] [--repeats 3]
    --rehearse: tiny tables on the CPU back-end, fp32, short windows: checks the plumbing (its rates are not measurements and say so).
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
# name -> (model, batch, precision, stream group, per-bank indices)
SHAPES = {"A256_fp32_g64": ("A", 256, "fp32", 64, False), "A256_fp32_g16": ("A", 256, "fp32", 16, False), "B1024_bf16_g128": ("B", 1024, "bf16", 128, False),
          "C4096_bank_bf16": ("C", 4096, "bf16", 1, True), "C4096_bank_fp8": ("C", 4096, "fp8", 1, True)}
NBUF = 8


def leg(args):
    """One (shape, setting) in this process: JSON on the last line of stdout."""
    import __graft_entry__ as graft
    fr = graft.load_package()
    which, B, prec, group, bank = SHAPES[args.shape]
    device = -1 if args.rehearse else 0
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("fc_epilogue_bench: no MI355X visible -- a timing needs the GPU")
    model = fr.Model.builtin({"A": fr.MODEL_A, "B": fr.MODEL_B, "C": fr.MODEL_C}[which])
    kw = {"index_mode": fr.INDEX_PER_BANK} if bank else {}
    if args.rehearse:
        B, kw["max_rows"] = min(B, 32), 2000
    model = model.clone(**kw) if kw else model
    ctx = fr.Context(model, device=device)
    ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
    if prec != "fp32" and not args.rehearse:
        ctx.set_fc_precision(fr.FC_BF16 if prec == "bf16" else fr.FC_FP8)
    rng = np.random.default_rng(4242)
    fc = list(model.fc)
    if args.setting == "epilogue":
        for l in range(4):
            ctx.set_epilogue(l, (rng.random(fc[l + 1]).astype(np.float32) * 2 - 1) / np.float32(np.sqrt(fc[l])), "relu" if l < 3 else "none")
    ctx.set_stream_group(group)
    ranges = model.index_ranges()
    wk = fr.Worker(ctx, B)
    host_idx = [(rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32) for _ in range(NBUF)]
    host_dense = [rng.uniform(-1, 1, (B, model.dense_len)).astype(np.float32) for _ in range(NBUF)] if model.dense_len else None
    if prec == "fp8" and not args.rehearse:
        wk.calibrate_fp8(host_idx[0], host_dense[0] if host_dense else None)
    idx = [fr.DeviceBuffer.from_numpy(ctx, a) for a in host_idx]
    dense = [fr.DeviceBuffer.from_numpy(ctx, a) for a in host_dense] if host_dense else None
    scores = [fr.DeviceBuffer(ctx, B * 4) for _ in range(NBUF)]
    LIST = max(group, 16)
    ks = [i % NBUF for i in range(LIST)]
    plist = wk.make_push_list([B] * LIST, [idx[k] for k in ks], [dense[k] for k in ks] if dense else None, [scores[k] for k in ks])

    def run(n):
        for _ in range(max(1, n // LIST)):
            wk.push_device_list(plist)
        wk.sync()
    run(2 * LIST)   # warm-up: code objects, the tables' first touch, the chain width
    kernel = wk.last_kernel()
    layers = []
    if group == 1 and not args.rehearse:   # the chain's layers are launches of their own: name each
        for l in range(4):
            wk.fc_layer_only(B, l)
            layers.append(wk.last_kernel())
            wk.sync()
    t0 = time.perf_counter()
    run(4 * LIST)
    per = (time.perf_counter() - t0) / (4 * LIST)
    n = max(LIST, int(args.seconds / per) // LIST * LIST)
    rates = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        run(n)
        rates.append(n * B / (time.perf_counter() - t0))
    wk.close()
    ctx.close()
    print(json.dumps({"shape": args.shape, "setting": args.setting, "kernel": kernel, "layer_kernels": layers, "batches_per_window": n,
                      "inferences_per_s": [round(r) for r in rates]}), flush=True)


def child(args, shape, setting, limit=240):
    """One leg as a child process in a session of its own -> (result or None, error text or None)."""
    cmd = [sys.executable, os.path.abspath(__file__), "--leg", "--shape", shape, "--setting", setting, "--seconds", str(args.seconds), "--repeats", str(args.repeats)]
    if args.rehearse:
        cmd.append("--rehearse")
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    if setting == "parent":
        env["FR_LIB"] = os.path.abspath(args.parent_lib)
    p = subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, start_new_session=True, env=env)
    try:
        out, err = p.communicate(timeout=limit)
    except subprocess.TimeoutExpired:
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        return None, "%s / %s ran into its time limit of %d s" % (shape, setting, limit)
    if p.returncode != 0:
        return None, "%s / %s exited with status %d: %s" % (shape, setting, p.returncode, err.decode()[-400:])
    return json.loads(out.decode().strip().splitlines()[-1]), None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fc_epilogue.json"))
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--leg", action="store_true")
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--setting", choices=("none", "epilogue", "parent"))
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    if args.leg:
        return leg(args)
    rows, error = {}, None
    for shape in SHAPES:
        if args.rehearse and SHAPES[shape][2] != "fp32":
            continue
        row = {}
        for _ in range(max(1, args.rounds)):
            for setting in (("parent",) if args.parent_lib else ()) + ("none", "epilogue"):
                res, error = child(args, shape, setting)
                if error:
                    break
                if setting in row:   # a later round: the same kernel, more windows
                    if res["kernel"] != row[setting]["kernel"]:
                        error = "%s / %s ran %s in one round and %s in another" % (shape, setting, row[setting]["kernel"], res["kernel"])
                        break
                    row[setting]["inferences_per_s"] += res["inferences_per_s"]
                else:
                    row[setting] = res
            if error:
                break
        if error:
            break
        med = {s: float(np.median(row[s]["inferences_per_s"])) for s in row}
        row["ratio_epilogue_over_none"] = round(med["epilogue"] / med["none"], 4)
        if "parent" in med:
            row["ratio_none_over_parent"] = round(med["none"] / med["parent"], 4)
            row["none_not_below_parent_lowest_window"] = bool(med["none"] >= min(row["parent"]["inferences_per_s"]))
        rows[shape] = row
        print("%-18s none %8.1f M inf/s (%s)  epilogue %8.1f M inf/s (%s)  ratio %.3f%s" % (
            shape, med["none"] / 1e6, row["none"]["kernel"], med["epilogue"] / 1e6, row["epilogue"]["kernel"], row["ratio_epilogue_over_none"],
            "  none / parent %.3f" % row["ratio_none_over_parent"] if "parent" in med else ""), flush=True)
    doc = {}
    if os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc["epilogue_cost"] = {"what": __doc__.strip().splitlines()[0], "rehearsal_not_a_measurement": bool(args.rehearse), "seconds_per_window": args.seconds, "rounds_in_alternation": max(1, args.rounds),
                            "shapes": rows, "stopped_at": error}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if error:
        sys.exit("fc_epilogue_bench: " + error)


if __name__ == "__main__":
    main()

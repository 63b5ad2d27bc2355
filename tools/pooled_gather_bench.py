#!/usr/bin/env python3
"""The pooled gather against the one-hot gather, in one process on one MI355X -> profiles/pooled_gather.json.

Model-C (full size), batch 4096, FR_FILL_HASH, uniform random indices, FR_INDEX_PER_TABLE and FR_INDEX_PER_BANK.  Per mode:
  * fr_worker_gather_only (gather_pack_stream_kernel, unchanged): the yardstick, taken in the same process so that box-to-box
    spread drops out, and
  * fr_worker_gather_pooled at uniform hots = 1, 2, 4, 8, 16 (every slot filled),
every shape warmed up first, each timed window `--reps` launches between two HIP events on the worker's stream
(Worker.timer_start / timer_stop_ms), the yardstick and the pooled forms alternated for `--rounds` rounds so that the file carries the
spread as well as the medians.  Index buffers rotate: 4 .. 32 per shape, as many as bring their index bytes to 512 MB (per-bank rows are
short: 32 buffers).  With the row lines a batch touches (4096 items x 82 .. 376 columns x hots slots x 128 bytes: 43 MB .. 3 GB per
buffer) the buffers of every shape together exceed the 256 MB Infinity Cache, as bench.py's rotating buffers have since round 6.

Reported per shape: us per batch, row words (16 bytes) fetched per second, algorithmic TB/s = (fetched row bytes + record bytes + dense
bytes + index bytes) / time.  Expectation recorded (not asserted): at hots >= 4 the fetched-row rate does not fall below 0.9 x the
one-hot kernel's of the same run.

    python tools/pooled_gather_bench.py [--modes table,bank] [--hots 1,2,4,8,16] [--reps 400] [--rounds 3] [--out profiles/pooled_gather.json]
    --pool sum[,mean,weighted]: the folds to time at every hots (default sum, the shapes "pooled_hotsN" as ever; "mean_hotsN": every column
    FR_POOL_MEAN; "weighted_hotsN": fr_worker_gather_pooled_weighted with a float32 weight per slot in (0.5, 1.5), one weight buffer per index
    buffer -- the weighted fold reads 4 more bytes per slot, counted in its algorithmic bytes).  FR_LIB=<another build of the same ABI> times
    that build (an A/B run against an older commit can only ask it for the folds it has).
    --rehearse: tiny tables on the CPU back-end, to check the plumbing without a GPU (its times are not measurements and say so).
    --csr: the offsets (CSR) form against the padded form on the SAME bags -> profiles/pooled_gather_csr.json.  Caps 16 and 64 (--caps), two seeded
    bag-length laws: "full" (every bag at the cap) and "skewed" (a geometric law clipped to the cap, mean about cap / 8, empty bags included);
    unweighted SUM, plus the weighted fold at cap 16.  The padded buffers hold the bags padded with -1, the offsets-form buffers the same bags
    compacted (fleetrec_amd.bags_to_csr); the two forms alternate within every round.  Per shape: us per batch, fetched row words per second (the
    bags' non-empty entries x the words of their rows), algorithmic bytes (rows + records + dense + indices + offsets + weights) and TB/s, the
    spread between rounds; per pair the offsets form's time over the padded form's.
Experiments build (FR_LIB=.../libfleetrec_exp.so): --sweep times FR_POOL_WIN x FR_POOL_ITEMS instead (profiles/pooled_gather_window_sweep.md).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as graft  # noqa: E402

HBM_PEAK_TBS = 8.0
SEED_TABLES = 0xF1EE7


def table_words(model):
    """16-byte TABLE / COPY words and dense floats of one record."""
    tw = sum(s.len // 4 for s in model.segments() if s.kind != 2)
    return tw, model.dense_len


def make_buffers(fr, ctx, model, rng, B, hots, min_bytes):
    ranges = model.index_ranges()
    P = len(ranges) * hots
    nbuf = max(4, min(32, -(-min_bytes // (B * P * 4))))
    bufs = []
    for _ in range(nbuf):
        a = (rng.random((B, len(ranges), hots)) * ranges[None, :, None]).astype(np.int32).reshape(B, P)
        bufs.append(fr.DeviceBuffer.from_numpy(ctx, a))
    return bufs


def window(wk, launch, bufs, dns, reps, offset):
    wk.timer_start()
    for i in range(reps):
        k = (offset + i) % len(bufs)
        launch(bufs[k], dns[k % len(dns)] if dns else None)
    ms = wk.timer_stop_ms()
    wk.sync()
    return ms * 1e3 / reps   # us per batch


def run_mode(fr, args, mode_name, device, rehearse):
    imode = {"table": fr.INDEX_PER_TABLE, "bank": fr.INDEX_PER_BANK}[mode_name]
    base = fr.Model.builtin(fr.MODEL_C)
    model = base.clone(max_rows=2000, index_mode=imode) if rehearse else base.clone(index_mode=imode)
    B = args.batch
    ctx = fr.Context(model, device=device)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    rng = np.random.default_rng(20260 + imode)
    wk = fr.Worker(ctx, B)
    rec = wk.records_dptr()
    tw, dense_len = table_words(model)
    K = model.record_len
    dns = [fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (B, dense_len)).astype(np.float32)) for _ in range(4)] if dense_len else None
    min_bytes = (1 << 20) if rehearse else (512 << 20)
    shapes = {}   # name -> (launch, bufs, hots or 0)
    one_bufs = make_buffers(fr, ctx, model, rng, B, 1, min_bytes)
    shapes["gather_only"] = (lambda i, d: wk.gather_only(B, i, d, rec), one_bufs, 0)
    fold_of = {"gather_only": "sum"}
    for h in args.hots:
        bufs = one_bufs if h == 1 else make_buffers(fr, ctx, model, rng, B, h, min_bytes)
        for pool in args.pool:
            name = ("pooled" if pool == "sum" else pool) + "_hots%d" % h
            fold_of[name] = pool
            if pool == "weighted":   # a weight buffer per index buffer, found through the index buffer's address
                wts = {b.ptr.value: fr.DeviceBuffer.from_numpy(ctx, rng.uniform(0.5, 1.5, (B, model.idx_cols * h)).astype(np.float32)) for b in bufs}
                shapes[name] = (lambda i, d, wts=wts: wk.gather_pooled(B, i, d, rec, weights=wts[i.ptr.value]), bufs, h)
            else:
                shapes[name] = (lambda i, d: wk.gather_pooled(B, i, d, rec), bufs, h)
    kernels, times = {}, {n: [] for n in shapes}

    def select(name, h):
        ctx.set_pooling(np.full(model.idx_cols, h, np.int32) if h else None)
        if fold_of[name] == "mean":
            ctx.set_pooling_modes(np.full(model.idx_cols, fr.POOL_MEAN, np.int32))

    for name, (launch, bufs, h) in shapes.items():   # warm-up of every shape: code objects, the tables' first touch
        select(name, h)
        window(wk, launch, bufs, dns, min(args.reps, 4 * len(bufs)), 0)
        kernels[name] = wk.last_kernel()
    for r in range(args.rounds):
        for name, (launch, bufs, h) in shapes.items():
            select(name, h)
            times[name].append(window(wk, launch, bufs, dns, args.reps, r * args.reps))
    select("gather_only", 0)
    out = {"index_mode": mode_name, "index_cols": int(model.idx_cols), "record_floats": int(K), "table_words_per_record": int(tw), "shapes": {}}
    t0 = float(np.median(times["gather_only"]))
    for name, (launch, bufs, h) in shapes.items():
        slots = max(h, 1)
        us = float(np.median(times[name]))
        fetched = B * tw * slots
        by = fetched * 16 + B * K * 4 + B * dense_len * 4 + B * model.idx_cols * slots * 4 * (2 if fold_of[name] == "weighted" else 1)
        e = {"kernel": kernels[name], "hots": h, "pool": fold_of[name], "index_buffers": len(bufs), "index_bytes_per_batch": B * model.idx_cols * slots * 4,
             "us_per_batch_rounds": [round(t, 3) for t in times[name]], "us_per_batch": round(us, 3),
             "row_words_fetched_per_s": fetched / (us * 1e-6), "algorithmic_bytes_per_batch": by, "algorithmic_TBs": by / (us * 1e-6) / 1e12,
             "frac_of_8TBs": by / (us * 1e-6) / 1e12 / HBM_PEAK_TBS}
        if h:
            e["row_rate_vs_gather_only"] = (fetched / us) / (B * tw / t0)
            if h >= 4:
                e["expectation_row_rate_ge_0.9x_one_hot"] = bool(e["row_rate_vs_gather_only"] >= 0.9)
        out["shapes"][name] = e
        print("%-5s %-14s %9.2f us  %7.2f G row words/s  %5.2f TB/s  %s  %s" % (mode_name, name, us, e["row_words_fetched_per_s"] / 1e9, e["algorithmic_TBs"],
                                                                             ("x%.2f rows/s of one-hot" % e["row_rate_vs_gather_only"]) if h else "", kernels[name]), flush=True)
    wk.close()
    ctx.close()
    return out


def bag_lengths(rng, law, B, cols, cap):
    """int64 [B][cols].  full: the cap.  skewed: geometric on 0, 1, 2, ... with mean cap / 8, clipped to the cap (a long tail, empty bags included)."""
    if law == "full":
        return np.full((B, cols), cap, np.int64)
    mean = cap / 8.0
    return np.minimum(rng.geometric(1.0 / (1.0 + mean), size=(B, cols)) - 1, cap)


def run_csr(fr, args, mode_name, device, rehearse):
    imode = {"table": fr.INDEX_PER_TABLE, "bank": fr.INDEX_PER_BANK}[mode_name]
    base = fr.Model.builtin(fr.MODEL_C)
    model = base.clone(max_rows=2000, index_mode=imode) if rehearse else base.clone(index_mode=imode)
    B, C = args.batch, model.idx_cols
    ctx = fr.Context(model, device=device)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    rng = np.random.default_rng(20270 + imode)
    ranges = model.index_ranges()
    words_of_col = np.zeros(C, np.int64)   # 16-byte TABLE / COPY words of a record that every entry of the column's bag fetches
    bank_of = model.bank_map()[0] if imode == fr.INDEX_PER_BANK else None
    for sg in model.segments():
        if sg.kind != 2:
            words_of_col[sg.src if bank_of is None else int(bank_of[sg.src])] += sg.len // 4
    K, dense_len = model.record_len, model.dense_len
    out = {"index_mode": mode_name, "index_cols": int(C), "record_floats": int(K), "shapes": {}, "pairs": {}}
    for cap in args.caps:
        ctx.set_pooling(np.full(C, cap, np.int32))
        wk = fr.Worker(ctx, B)
        rec = wk.records_dptr()
        dns = [fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (B, dense_len)).astype(np.float32)) for _ in range(4)] if dense_len else None
        nbuf = 2 if rehearse else max(2, min(4, -(-(512 << 20) // (B * C * cap * 4))))
        for law in ("full", "skewed"):
            folds = ["sum"] + (["weighted"] if cap == args.caps[0] else [])
            sets, nnz_sum, fetched = [], 0, 0
            for _ in range(nbuf):   # the same bags in both forms
                L = bag_lengths(rng, law, B, C, cap)
                rect = (rng.random((B, C, cap)) * ranges[None, :, None]).astype(np.int32)
                rect[np.arange(cap)[None, None, :] >= L[:, :, None]] = -1
                rect = rect.reshape(B, C * cap)
                w = rng.uniform(0.5, 1.5, rect.shape).astype(np.float32) if "weighted" in folds else None
                off, ind, wf = fr.bags_to_csr(rect, np.full(C, cap), weights=w)
                nnz_sum += int(ind.size)
                fetched += int((L * words_of_col[None, :]).sum())
                up = lambda a: fr.DeviceBuffer.from_numpy(ctx, a if a.size else np.zeros(1, a.dtype))
                sets.append({"rect": up(rect), "w": up(w) if w is not None else None, "off": up(off), "ind": up(ind), "wf": up(wf) if wf is not None else None,
                             "nnz": int(ind.size)})
            nnz, fetched = nnz_sum / nbuf, fetched / nbuf
            shapes = {}
            for fold in folds:
                wt = fold == "weighted"
                shapes["%s_cap%d_%s_padded" % (fold, cap, law)] = (
                    lambda s, d, wt=wt: wk.gather_pooled(B, s["rect"], d, rec, weights=s["w"] if wt else None), "padded", fold)
                shapes["%s_cap%d_%s_offsets" % (fold, cap, law)] = (
                    lambda s, d, wt=wt: wk.gather_pooled_csr(B, s["off"], s["ind"], s["nnz"], d, rec, weights=s["wf"] if wt else None), "offsets", fold)
            kernels, times = {}, {n: [] for n in shapes}
            for name, (launch, form, fold) in shapes.items():   # warm-up of every shape
                window(wk, launch, sets, dns, min(args.reps, 4 * nbuf), 0)
                kernels[name] = wk.last_kernel()
            for r in range(args.rounds):   # the two forms alternate within a round
                for name, (launch, form, fold) in shapes.items():
                    times[name].append(window(wk, launch, sets, dns, args.reps, r * args.reps))
            for name, (launch, form, fold) in shapes.items():
                us = float(np.median(times[name]))
                wt = 2 if fold == "weighted" else 1
                idx_bytes = (B * C * cap * 4 * wt) if form == "padded" else (nnz * 4 * wt + (B * C + 1) * 4)
                by = fetched * 16 + B * K * 4 + B * dense_len * 4 + idx_bytes
                out["shapes"][name] = {"kernel": kernels[name], "cap": cap, "law": law, "form": form, "pool": fold, "buffer_sets": nbuf, "mean_bag_length": nnz / (B * C),
                                       "index_offsets_weights_bytes_per_batch": idx_bytes, "us_per_batch_rounds": [round(t, 3) for t in times[name]],
                                       "us_per_batch": round(us, 3), "us_spread_max_minus_min": round(max(times[name]) - min(times[name]), 3),
                                       "row_words_fetched_per_s": fetched / (us * 1e-6), "algorithmic_bytes_per_batch": by, "algorithmic_TBs": by / (us * 1e-6) / 1e12}
                print("%-5s %-34s %10.2f us  %7.2f G row words/s  %5.2f TB/s  %s" % (mode_name, name, us, fetched / (us * 1e-6) / 1e9, by / (us * 1e-6) / 1e12,
                                                                                 kernels[name]), flush=True)
            for fold in folds:
                pn, on = "%s_cap%d_%s_padded" % (fold, cap, law), "%s_cap%d_%s_offsets" % (fold, cap, law)
                tp, to = times[pn], times[on]
                out["pairs"]["%s_cap%d_%s" % (fold, cap, law)] = {
                    "offsets_over_padded": float(np.median(to) / np.median(tp)),
                    "offsets_median_below_padded_median_minus_padded_spread": bool(np.median(to) < np.median(tp) - (max(tp) - min(tp)))}
            for s_ in sets:
                for b in s_.values():
                    if isinstance(b, fr.DeviceBuffer):
                        b.free()
        wk.close()
    ctx.close()
    return out


def run_sweep(fr, args, device):
    """Experiments build: FR_POOL_WIN x FR_POOL_ITEMS at every hots, per-bank and per-table -> a markdown table on stdout."""
    combos = [(1, 4), (1, 8), (2, 2), (2, 4), (2, 8), (4, 1), (4, 2), (4, 4), (4, 8), (8, 1), (8, 2), (8, 4), (16, 1), (16, 2)]
    rows = []
    for mode_name in args.modes:
        imode = {"table": fr.INDEX_PER_TABLE, "bank": fr.INDEX_PER_BANK}[mode_name]
        model = fr.Model.builtin(fr.MODEL_C).clone(index_mode=imode)
        ctx = fr.Context(model, device=device)
        ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
        rng = np.random.default_rng(7)
        B = args.batch
        wk = fr.Worker(ctx, B)
        rec = wk.records_dptr()
        dns = [fr.DeviceBuffer.from_numpy(ctx, rng.uniform(-1, 1, (B, model.dense_len)).astype(np.float32)) for _ in range(4)]
        for h in args.hots:
            bufs = make_buffers(fr, ctx, model, rng, B, h, 512 << 20)
            ctx.set_pooling(np.full(model.idx_cols, h, np.int32))
            launch = lambda i, d: wk.gather_pooled(B, i, d, rec)
            for win, items in combos:
                if win > max(h, 1) * 2 and win > 1:
                    continue
                os.environ["FR_POOL_WIN"], os.environ["FR_POOL_ITEMS"] = str(win), str(items)
                window(wk, launch, bufs, dns, 3 * len(bufs), 0)
                us = [window(wk, launch, bufs, dns, args.reps, r * args.reps) for r in range(args.rounds)]
                rows.append((mode_name, h, win, items, float(np.median(us)), min(us), max(us), wk.last_kernel()))
                print("| %s | %d | %d | %d | %.2f | %.2f | %.2f | %s |" % rows[-1], flush=True)
            ctx.set_pooling(None)
            for b in bufs:
                b.free()
        wk.close()
        ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="table,bank")
    ap.add_argument("--hots", default="1,2,4,8,16")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooled_gather.json"))
    ap.add_argument("--pool", default="sum")
    ap.add_argument("--rehearse", action="store_true")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--csr", action="store_true")
    ap.add_argument("--caps", default="16,64")
    args = ap.parse_args()
    args.modes = [m for m in args.modes.split(",") if m]
    args.hots = [int(h) for h in args.hots.split(",") if h]
    args.pool = [p for p in args.pool.split(",") if p]
    if not args.pool or any(p not in ("sum", "mean", "weighted") for p in args.pool):
        sys.exit("--pool: a comma-separated list of sum, mean, weighted")
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("pooled_gather_bench: no MI355X visible -- a timing needs the GPU (--rehearse checks the plumbing on the CPU back-end)")
    device = -1 if args.rehearse else 0
    if args.sweep:
        if "FR_LIB" not in os.environ:
            sys.exit("--sweep needs the experiments build: FR_LIB=.../libfleetrec_exp.so (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
        print("| mode | hots | window | items | us median | min | max | kernel |\n|---|---|---|---|---|---|---|---|", flush=True)
        run_sweep(fr, args, device)
        return
    if args.csr:
        args.caps = [int(c) for c in args.caps.split(",") if c]
        if args.out == ap.get_default("out"):
            args.out = os.path.join(ROOT, "profiles", "pooled_gather_csr.json")
        t_start = time.time()
        res = {"tool": "tools/pooled_gather_bench.py --csr", "model": "C", "batch": args.batch, "fill": "FR_FILL_HASH", "index_law": "uniform rows; bag lengths: full / skewed (clipped geometric, mean cap / 8)",
               "timed_launches_per_window": args.reps, "rounds": args.rounds, "caps": args.caps, "library": os.environ.get("FR_LIB", "libfleetrec.so"),
               "timing": "HIP events on the worker's stream around each window; the padded and the offsets form alternate within a round; median over the rounds",
               "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "modes": [run_csr(fr, args, m, device, args.rehearse) for m in args.modes]}
        res["wall_s"] = round(time.time() - t_start, 1)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print("wrote", args.out)
        return
    t_start = time.time()
    res = {"tool": "tools/pooled_gather_bench.py", "model": "C", "batch": args.batch, "fill": "FR_FILL_HASH", "index_law": "uniform", "timed_launches_per_window": args.reps,
           "rounds": args.rounds, "pool": args.pool, "library": os.environ.get("FR_LIB", "libfleetrec.so"), "timing": "HIP events on the worker's stream around each window; median over the rounds", "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse),
           "modes": [run_mode(fr, args, m, device, args.rehearse) for m in args.modes]}
    res["wall_s"] = round(time.time() - t_start, 1)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()

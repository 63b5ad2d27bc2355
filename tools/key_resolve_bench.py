#!/usr/bin/env python3
"""Keyed lookups on one MI355X -> profiles/key_resolve.json.

  (a) resolve  HIP-event time of fr_worker_resolve_keys_device alone beside fr_worker_gather_only for the same batch in the same process (the gather is
               the parent commit's kernel, unchanged): `--calls` calls back to back between two events on the worker's stream, `--repeats` windows
               after a warm-up, microseconds per call; the key buffers rotate (8 batches of different keys), the gather reads the rows the resolve
               wrote.  Configurations: Model-A batch 256 with every column MAPPED and every row keyed; Model-C batch 4096 per bank with every column
               MAPPED (up to --max-keys keys per bank: the maps together are many times the Infinity Cache); Model-C batch 4096 per table with every
               column HASHED (full maps for its 376 tables would not fit beside 63 GB of tables).  Every looked-up key is present.  Beside the times:
               keys and slot bytes, the fabric requests a lookup costs at least (one 16-byte slot read per key + the key's own 8 bytes, streamed), and
               the probes per lookup -- 1 + the mean displacement of the keys of the largest map, from a host-side replay of linear probing (the sum
               of displacements does not depend on the order in which the device claimed the slots).
  (b) submit   Model-A (full size), host clock per batch with the pinned buffers already filled: fr_worker_submit_keyed + sync against
               fr_worker_submit + sync on the rows the same keys resolve to, alternating, at batch 256 and 4096; the scores are compared bit for bit.

One GPU process at a time: every leg is a child process under its own time limit and in a process group of its own (killed whole at the limit); the
first child that runs into its limit or exits with a non-zero status ends the tool -- what was measured is written, nothing more is started on the
card, the exit status is non-zero.

    python tools/key_resolve_bench.py [--legs resolve,submit] [--out profiles/key_resolve.json]
    --rehearse: the CPU back-end, small shapes, host clock: checks the plumbing (its times are not measurements and say so).
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
ROTATE = 8
ODD = np.uint64(0x9E3779B97F4A7C15)


def _fr(args):
    import __graft_entry__ as graft
    fr = graft.load_package()
    if not args.rehearse and fr.device_count() < 1:
        sys.exit("key_resolve_bench: no MI355X visible -- a timing needs the GPU")
    return fr


def mix64(z):
    z = z.astype(np.uint64)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xbf58476d1ce4e5b9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def key_of(rows, col):
    """the key of row `rows` of column col: a bijection of the row number, spread over 64 bits (never -1 for the rows used here)"""
    return ((rows.astype(np.uint64) + np.uint64(1)) * ODD + np.uint64(col)).view(np.int64)


def probes_per_lookup(keys, seed, slots):
    """1 + the mean displacement of `keys` in a linear-probing table of `slots` slots: a replay in rounds -- every pending key tries its slot, one
    key per free slot wins, the others move on"""
    pos = (mix64(keys.view(np.uint64) ^ np.uint64(seed)) & np.uint64(slots - 1)).astype(np.int64)
    taken = np.zeros(slots, bool)
    pending = np.arange(keys.size)
    moved = 0
    while pending.size:
        p = pos[pending]
        free = ~taken[p]
        _, first = np.unique(p[free], return_index=True)
        won = pending[free][first]
        taken[pos[won]] = True
        keep = np.ones(pending.size, bool)
        keep[np.flatnonzero(free)[first]] = False
        pending = pending[keep]
        pos[pending] = (pos[pending] + 1) & (slots - 1)
        moved += pending.size
    return 1.0 + moved / keys.size


def timed(fr, wk, calls, repeats, rehearse, fn):
    for i in range(2 * ROTATE):
        fn(i)
    wk.sync()
    us = []
    for _ in range(repeats):
        if rehearse:
            t0 = time.perf_counter()
            for i in range(calls):
                fn(i)
            wk.sync()
            us.append(round(1e6 * (time.perf_counter() - t0) / calls, 3))
            continue
        wk.timer_start()
        for i in range(calls):
            fn(i)
        ms = wk.timer_stop_ms()
        wk.sync()
        us.append(round(1e3 * ms / calls, 3))
    return us


def leg_resolve(args):
    fr = _fr(args)
    device = -1 if args.rehearse else 0
    rng = np.random.default_rng(91)
    out = {"leg": "resolve", "configs": []}
    configs = (("A", None, 256, fr.KEYS_MAPPED), ("C", fr.INDEX_PER_BANK, 4096, fr.KEYS_MAPPED), ("C", None, 4096, fr.KEYS_HASHED))
    for which, index_mode, batch, mode in configs:
        m = fr.Model.builtin(fr.MODEL_A if which == "A" else fr.MODEL_C)
        if index_mode is not None or args.rehearse:
            m = m.clone(index_mode=index_mode, max_rows=2000 if args.rehearse else 0)
        ctx = fr.Context(m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
        C, ranges = m.idx_cols, np.asarray(m.index_ranges(), np.int64)
        n_keys = np.minimum(ranges, args.max_keys)
        slot_bytes, probes = 0, None
        for c in range(C):
            if mode == fr.KEYS_HASHED:
                ctx.set_key_space(c, mode, seed=1000 + c)
                continue
            ctx.set_key_space(c, mode, seed=1000 + c, max_keys=int(n_keys[c]), miss_row=0)
            slots = 2
            while slots < 2 * int(n_keys[c]):
                slots *= 2
            slot_bytes += 16 * slots
            for r0 in range(0, int(n_keys[c]), 1 << 20):
                rows = np.arange(r0, min(r0 + (1 << 20), int(n_keys[c])), dtype=np.int64)
                ctx.put_keys(c, key_of(rows, c), rows.astype(np.int32))
            if c == int(np.argmax(n_keys)):
                probes = round(probes_per_lookup(key_of(np.arange(int(n_keys[c]), dtype=np.int64), c), 1000 + c, slots), 4)
        wk = fr.Worker(ctx, batch)
        d_keys, d_rows = [], []
        for _ in range(ROTATE):
            rows = (rng.random((batch, C)) * n_keys[None, :]).astype(np.int64)
            keys = np.stack([key_of(rows[:, c], c) for c in range(C)], axis=1) if mode == fr.KEYS_MAPPED else rng.integers(-2 ** 63, 2 ** 63 - 1, size=(batch, C), dtype=np.int64)
            d_keys.append(fr.DeviceBuffer.from_numpy(ctx, keys))
            d_rows.append(fr.DeviceBuffer(ctx, batch * C * 4))
        d_dense = fr.DeviceBuffer.from_numpy(ctx, rng.standard_normal((batch, m.dense_len)).astype(np.float32)) if m.dense_len else None
        d_rec = fr.DeviceBuffer(ctx, batch * m.record_len * 4)
        resolve = lambda i: wk.resolve_keys_device(batch, d_keys[i % ROTATE], d_rows[i % ROTATE])
        gather = lambda i: wk.gather_only(batch, d_rows[i % ROTATE], d_dense, d_rec)
        us_r = timed(fr, wk, args.calls, args.repeats, args.rehearse, resolve)
        us_g = timed(fr, wk, args.calls, args.repeats, args.rehearse, gather)
        if mode == fr.KEYS_MAPPED:   # every key was present: the rows are the bijection's
            got = d_rows[0].download(np.int32, batch * C).reshape(batch, C)
            assert wk.key_misses() == 0 and (got >= 0).all() and (got < n_keys[None, :]).all()
        lookups = batch * C
        med_r, med_g = float(np.median(us_r)), float(np.median(us_g))
        out["configs"].append({"model": which, "index_mode": {None: "model's own", fr.INDEX_PER_BANK: "per bank"}[index_mode], "batch": batch,
                               "mode": {fr.KEYS_MAPPED: "MAPPED", fr.KEYS_HASHED: "HASHED"}[mode], "index_columns": C, "lookups_per_batch": lookups,
                               "keys_in_maps": int(n_keys.sum()) if mode == fr.KEYS_MAPPED else 0, "slot_bytes": slot_bytes, "probes_per_lookup": probes,
                               "fabric_requests_per_batch_at_least": lookups + lookups * 8 // 128 if mode == fr.KEYS_MAPPED else lookups * 8 // 128,
                               "resolve_us_per_call": us_r, "gather_only_us_per_call": us_g, "median_us": {"resolve": med_r, "gather_only": med_g},
                               "lookups_per_us": round(lookups / med_r, 1) if med_r > 0 else None, "resolve_slower_than_its_gather": bool(med_r > med_g)})
        for b in d_keys + d_rows + [d_dense, d_rec]:
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
    C, ranges = m.idx_cols, np.asarray(m.index_ranges(), np.int64)
    n_keys = np.minimum(ranges, args.max_keys)
    for c in range(C):
        ctx.set_key_space(c, fr.KEYS_MAPPED, seed=1000 + c, max_keys=int(n_keys[c]), miss_row=0)
        for r0 in range(0, int(n_keys[c]), 1 << 20):
            rows = np.arange(r0, min(r0 + (1 << 20), int(n_keys[c])), dtype=np.int64)
            ctx.put_keys(c, key_of(rows, c), rows.astype(np.int32))
    rng = np.random.default_rng(92)
    out = {"leg": "submit", "model": "A", "mode": "MAPPED", "batches": []}
    for B in (256, 4096):
        wk = fr.Worker(ctx, B)
        rows = (rng.random((B, C)) * n_keys[None, :]).astype(np.int64)
        wk.key_rows()[:B * C] = np.stack([key_of(rows[:, c], c) for c in range(C)], axis=1).ravel()
        wk.idx[:B] = rows.astype(np.int32)

        def keyed():
            wk.submit_keyed(B, 0)
            wk.sync()

        def plain():
            wk.submit(B)
            wk.sync()

        sides = {"submit_keyed": keyed, "submit": plain}
        scores, us = {}, {k: [] for k in sides}
        for name, fn in sides.items():
            for _ in range(20):
                fn()
            scores[name] = wk.score[:B].copy().view(np.uint32)
        for _ in range(args.repeats):
            for name, fn in sides.items():     # alternating
                fn()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    fn()
                us[name].append(round(1e6 * (time.perf_counter() - t0) / args.calls, 2))
        out["batches"].append({"batch": B, "us_per_batch": us, "median_us": {k: float(np.median(v)) for k, v in us.items()},
                               "scores_equal_bit_for_bit": bool(np.array_equal(scores["submit_keyed"], scores["submit"]))})
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="")
    ap.add_argument("--legs", default="resolve,submit")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-keys", type=int, default=1 << 22, help="keys per MAPPED column at most (a column with fewer rows keys every row)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "key_resolve.json"))
    ap.add_argument("--rehearse", action="store_true")
    args = ap.parse_args()
    if args.leg == "resolve":
        return leg_resolve(args)
    if args.leg == "submit":
        return leg_submit(args)
    res = {"tool": "tools/key_resolve_bench.py", "options": {"legs": args.legs, "calls": args.calls, "repeats": args.repeats, "max_keys": args.max_keys},
           "one_gpu_process_at_a_time": True, "rehearsal_on_cpu_not_a_measurement": bool(args.rehearse), "not_measured": {}}
    env = dict(os.environ)
    env.pop("FR_LIB", None)
    stopped = None
    for leg in [l for l in args.legs.split(",") if l]:
        if stopped:
            res["not_measured"][leg] = "not started: " + stopped
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(args.calls if not args.rehearse else 3), "--repeats", str(args.repeats),
               "--max-keys", str(args.max_keys)]
        out, err = child(cmd + (["--rehearse"] if args.rehearse else []), env, 420)
        lines = [ln for ln in (out or "").splitlines() if ln.startswith("{")]
        if not lines:
            stopped = "%s ended with: %s" % (leg, (err or "no result line").splitlines()[0][:200])
            res["not_measured"][leg] = err or "no result line"
            continue
        res[leg] = json.loads(lines[-1])
        print(leg, lines[-1][:800], flush=True)
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
        sys.exit("key_resolve_bench: stopped, nothing started after it -- " + stopped)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B of the table-sharded step's two exchange modes (fr_comm_set_exchange: all-gather vs all-to-all of the slices) through the C-ABI step
(fr_worker_submit_sharded on every rank, then fr_worker_sync on every rank), the modes alternating step by step in one process on the same
contexts and communicators.  Per leg and mode: median / min us per step (a host clock around the submits + syncs of all ranks, after a
warm-up), the slice bytes rank 0 received and sent (fr_comm_exchange_bytes: counted, not measured) and whether the two modes' scores are
bit-identical.  Legs:
  cpu : G = 8 CPU shard contexts, the in-process host exchange (row-capped Model-C, fp32, --cpu-batch)
  gpu : G = 2 and 8 shard contexts on ONE GPU, the staged exchange (Model-C, bf16, batch 4096) -- PCIe and host staging, not xGMI
Usage: exchange_ab.py [--legs cpu,gpu] [--steps 20] [--warmup 3] [--max-rows 0] [--cpu-batch 512] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g   # noqa: E402

fr = g.load_package()
SEED_TABLES, SEED_WEIGHTS = 0xF1EE7, 99


def run_leg(name, m, device, G, prec, B, steps, warmup):
    ctxs, wks, comms = [], [], []
    try:
        for r in range(G):
            c = fr.Context(m, device=device, shard_rank=r, n_shards=G)
            c.fill_tables(fr.FILL_HASH, SEED_TABLES)
            c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
            if prec != fr.FC_FP32:
                c.set_fc_precision(prec)
            ctxs.append(c)
            wks.append(fr.Worker(c, B))
        comms = fr.Comm.init_all(ctxs)
        rng = np.random.default_rng(4096 + G)
        idx = (rng.random((B, len(m.rows()))) * m.rows()[None, :]).astype(np.int32)
        dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
        for w in wks:
            w.idx[:B] = idx
            w.dense[:B] = dense
        modes = ("allgather", "alltoall")
        times = {md: [] for md in modes}
        scores, nbytes = {}, {}
        for i in range(warmup + steps):
            for md in modes:
                for cm in comms:
                    cm.set_exchange(md)
                t0 = time.perf_counter()
                for r in range(G):
                    wks[r].submit_sharded(comms[r], B)
                for r in range(G):
                    wks[r].sync()
                dt = time.perf_counter() - t0
                if i >= warmup:
                    times[md].append(dt * 1e6)
                scores[md] = [w.score[:B].copy() for w in wks]
                nbytes[md] = comms[0].exchange_bytes()
        equal = all(np.array_equal(a, b) for a, b in zip(scores["allgather"], scores["alltoall"]))
        equal &= all(np.array_equal(s, scores["allgather"][0]) for s in scores["allgather"])
        out = {"leg": name, "G": G, "batch": B, "precision": {0: "f32", 1: "bf16", 2: "fp8"}[prec], "steps": steps, "warmup": warmup,
               "scores_bit_identical": bool(equal)}
        for md in modes:
            t = np.array(times[md])
            out[md] = {"us_per_step_median": round(float(np.median(t)), 1), "us_per_step_min": round(float(t.min()), 1),
                       "rank0_received_bytes": nbytes[md][0], "rank0_sent_bytes": nbytes[md][1]}
        out["median_ratio_alltoall_over_allgather"] = round(out["alltoall"]["us_per_step_median"] / out["allgather"]["us_per_step_median"], 3)
        return out
    finally:
        for w in wks:
            w.close()
        for cm in comms:
            cm.close()
        for c in ctxs:
            c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="cpu,gpu")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-rows", type=int, default=0, help="row cap of the GPU legs' Model-C (0: full size, 63.2 GB)")
    ap.add_argument("--cpu-batch", type=int, default=512)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    legs = a.legs.split(",")
    results = []
    if "cpu" in legs:
        m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=2000)
        results.append(run_leg("cpu host exchange", m, fr.DEVICE_CPU, 8, fr.FC_FP32, a.cpu_batch, a.steps, a.warmup))
        print(json.dumps(results[-1]), flush=True)
    if "gpu" in legs:
        m = fr.Model.builtin(fr.MODEL_C)
        if a.max_rows:
            m = m.clone(max_rows=a.max_rows)
        for G in (2, 8):
            results.append(run_leg("staged on one GPU (PCIe + host staging, not xGMI)", m, 0, G, fr.FC_BF16, 4096, a.steps, a.warmup))
            print(json.dumps(results[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")
    return 0 if all(r["scores_bit_identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())

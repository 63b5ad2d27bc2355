"""Shared by tests/test_cpu_pooled_sharded.py and tests/test_gpu_pooled_sharded.py: multi-hot pooled lookups on table-sharded contexts
(include/fleetrec_serving.h: fr_ctx_create_sharded_pooled, fr_worker_gather_slices_pooled[_csr], fr_worker_submit_sharded_pooled[_csr],
fr_worker_calibrate_fp8_sharded_pooled).  device = -1: G CPU shard contexts on the in-process host exchange (fp32 only); device >= 0: G GPU
shard contexts of one device on the staged exchange.  Row-capped Model-C, batches 37 / 301 / 5 (5 < G = 8), workers of 1024 items.

Tolerances: none where both sides run the same code on the same bytes (slices, one live slot per bag, across ranks, offsets form against padded
form); 1e-5 / 3e-2 / 0.15 (fp32 against the unsharded pooled submit; bf16 / fp8 against tests/gpu_helpers.py's host restatements of the chains on
pooled records from the CPU back-end) -- the bounds tests/test_gpu_sharded.py uses for the one-hot step."""
import ctypes

import numpy as np
import pytest

import gather_matrix as GM
import pooled_helpers as P
from gpu_helpers import bf16_round, chain_bf16_reference, chain_fp8_reference, e4m3_encode, rel_err

CPU = -1
SEED_TABLES, SEED_WEIGHTS = P.SEED_TABLES, P.SEED_WEIGHTS
TOL = {"f32": 1e-5, "bf16": 3e-2, "fp8": 0.15}
CANARY = 0xA5
MAX_BATCH = 1024


def precision(fr, name):
    return {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[name]


def model_c(fr, device):
    return fr.Model.builtin(fr.MODEL_C).clone(max_rows=2000 if device == CPU else 5000)


def cycle(pattern, n_cols):
    return np.array([pattern[c % len(pattern)] for c in range(n_cols)], np.int32)


class Job:
    """G shard contexts of one row-capped Model-C on one device, pooling stated at creation (hots = None: created without), a worker and a
    communicator per rank; and (whole) an unsharded context with the same pooling set."""

    def __init__(self, fr, device, G, hots, modes=None, prec="f32", whole=True, comms=True):
        self.fr, self.device, self.G, self.hots, self.modes = fr, device, G, hots, modes
        self.m = m = model_c(fr, device)
        self.ctxs, self.wks, self.comms, self.whole, self.w0 = [], [], [], None, None
        try:
            for r in range(G):
                c = fr.Context(m, device=device, shard_rank=r, n_shards=G, hots=hots, modes=modes)
                self.ctxs.append(c)
                c.fill_tables(fr.FILL_HASH, SEED_TABLES)
                c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
                if prec != "f32":
                    c.set_fc_precision(precision(fr, prec))
                self.wks.append(fr.Worker(c, MAX_BATCH))
            if comms:
                self.comms = fr.Comm.init_all(self.ctxs)
            if whole:
                self.whole = fr.Context(m, device=device)
                self.whole.fill_tables(fr.FILL_HASH, SEED_TABLES)
                self.whole.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
                if hots is not None:
                    self.whole.set_pooling(hots, modes)
                self.w0 = fr.Worker(self.whole, MAX_BATCH)
        except Exception:
            self.close()
            raise

    def close(self):
        for w in self.wks + ([self.w0] if self.w0 else []):
            w.close()
        for cm in self.comms:
            cm.close()
        for c in self.ctxs + ([self.whole] if self.whole else []):
            c.close()
        self.wks, self.comms, self.ctxs, self.whole, self.w0 = [], [], [], None, None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def bags(self, rng, B, empty_share=0.2, empty_bags=4):
        return P.random_bags(rng, self.m.index_ranges(), self.hots, B, empty_share=empty_share, empty_bags=empty_bags)

    def dense(self, rng, B):
        return P.dense_for(rng, self.m, B)

    def set_exchange(self, mode):
        for cm in self.comms:
            cm.set_exchange(mode)

    def statuses(self, B, load, submit):
        """One step on every rank, submitted by one thread: load(wk) fills the pinned buffers, submit(wk, comm) enqueues.  -> (every rank's
        fr_worker_sync status, every rank's B scores)."""
        fr = self.fr
        for w in self.wks:
            load(w)
        for r in range(self.G):
            submit(self.wks[r], self.comms[r])
        st, got = [None] * self.G, [None] * self.G
        for r in reversed(range(self.G)):
            try:
                self.wks[r].sync()
                st[r] = fr.FR_OK
            except fr.FleetRecError as e:
                st[r] = e.status
            got[r] = self.wks[r].score[:B].copy()
        return st, got

    def step(self, B, load, submit):
        st, got = self.statuses(B, load, submit)
        assert st == [self.fr.FR_OK] * self.G, st
        for g in got[1:]:
            assert np.array_equal(g, got[0])          # every rank ends with the same B scores
        return got[0]

    def pooled_step(self, idx, dense, weights=None, csr=False):
        fr, B = self.fr, len(idx)
        wt = weights is not None
        if csr:
            off, ind, w = fr.bags_to_csr(idx, self.hots, weights)
            return self.step(B, lambda wk: wk.load_pooled_csr(off, ind, dense, w), lambda wk, cm: wk.submit_sharded_pooled_csr(cm, B, wt))
        return self.step(B, lambda wk: wk.load_pooled(idx, dense, weights), lambda wk, cm: wk.submit_sharded_pooled(cm, B, wt))

    def one_hot_step(self, idx, dense):
        B = len(idx)

        def load(wk):
            wk.idx[:B] = idx
            if wk.dense is not None:
                wk.dense[:B] = dense
        return self.step(B, load, lambda wk, cm: wk.submit_sharded(cm, B))

    def collective(self, fn):
        """fn(rank) on one thread per rank (the synchronous collectives)."""
        import threading
        errs = [None] * self.G

        def run(r):
            try:
                fn(r)
            except Exception as ex:   # noqa: BLE001
                errs[r] = ex
        th = [threading.Thread(target=run, args=(r,)) for r in range(self.G)]
        [t.start() for t in th]
        [t.join(120) for t in th]
        assert not any(t.is_alive() for t in th)
        assert errs == [None] * self.G, errs


def slice_bytes(fr, ctx, wk, hots, idx, dense, transport=None, weights=None, csr=False, shift=0):
    """The pooled slice of `idx` on one context -> (uint8 [B][row bytes], the gather's kernel name).  transport = None: fr_worker_gather_pooled*
    (fp32); else fr_worker_gather_slices_pooled[_csr].  The destination and a guard region behind it are filled with a canary first: nothing past
    batch x row bytes may change.  shift: the index rows (and weights) start that many bytes past a 16-byte boundary."""
    B = len(idx)
    esz = 4 if transport is None else {fr.FC_FP32: 4, fr.FC_BF16: 2, fr.FC_FP8: 1}[transport]
    row = ctx.shard_info()["slice_padded"] * esz
    guard = 4096
    bufs = []

    def dev(a):
        raw = fr.DeviceBuffer(ctx, a.nbytes + 256)
        bufs.append(raw)
        base = (raw.ptr.value + 15) // 16 * 16 + shift
        a = np.ascontiguousarray(a)
        if a.nbytes:
            fr._check(fr.lib().fr_memcpy_h2d(ctx._h, ctypes.c_void_p(base), a.ctypes.data_as(ctypes.c_void_p), a.nbytes))
        return base
    d_out = fr.DeviceBuffer.from_numpy(ctx, np.full(B * row + guard, CANARY, np.uint8))
    bufs.append(d_out)
    try:
        d_dense = dev(np.asarray(dense, np.float32)) if dense is not None else None
        if csr:
            off, ind, w = fr.bags_to_csr(idx, hots, weights)
            d_off, d_ind, d_w = dev(off), dev(ind), (dev(w) if w is not None else None)
            if transport is None:
                wk.gather_pooled_csr(B, d_off, d_ind, ind.size, d_dense, d_out, weights=d_w)
            else:
                wk.gather_slices_pooled_csr(B, d_off, d_ind, ind.size, d_dense, d_out, transport, weights=d_w)
        else:
            d_idx = dev(idx)
            d_w = dev(np.asarray(weights, np.float32)) if weights is not None else None
            if transport is None:
                wk.gather_pooled(B, d_idx, d_dense, d_out, weights=d_w)
            else:
                wk.gather_slices_pooled(B, d_idx, d_dense, d_out, transport, weights=d_w)
        name = wk.last_kernel()
        wk.sync()
        out = d_out.download(np.uint8, B * row + guard)
    finally:
        for b in bufs:
            b.free()
    assert (out[B * row:] == CANARY).all(), "bytes behind the batch's rows were written"
    return out[:B * row].reshape(B, row), name


def fold_inputs(job, rng, B, fold):
    """-> (idx, dense, weights or None, csr) of one fold kind: "sum" / "mean" (by the job's modes) / "weighted" / "csr" / "csr_weighted"."""
    idx = job.bags(rng, B)
    dense = job.dense(rng, B)
    weights = rng.uniform(0.25, 2.0, idx.shape).astype(np.float32) if "weighted" in fold else None
    return idx, dense, weights, fold.startswith("csr")


# ---- case 1: fp32 slices ---------------------------------------------------------------------------------------------------------------------
def check_fp32_slices(fr, device, pattern, fold, kernel=None):
    """G = 3: every rank's fr_worker_gather_pooled* slice [0, slice_len) equals columns [slice_offset, + slice_len) of an unsharded pooled
    context's records, bit for bit.  kernel: the shape the launch must name (GPU)."""
    G, B = 3, 37
    m = model_c(fr, device)
    hots = cycle(pattern, m.idx_cols)
    modes = cycle((fr.POOL_MEAN, fr.POOL_SUM, fr.POOL_MEAN), m.idx_cols) if fold == "mean" else None
    offs, lens, F = m.shard_plan(G)
    rng = np.random.default_rng(1000 + len(pattern) + 7 * int(max(pattern)))
    with Job(fr, device, G, hots, modes, comms=False) as job:
        idx, dense, weights, csr = fold_inputs(job, rng, B, fold)
        if csr:
            off, ind, w = fr.bags_to_csr(idx, hots, weights)
            want = job.w0.gather_pooled_csr_records(off, ind, dense, w).reshape(B, m.record_len)
            assert np.array_equal(want, job.w0.gather_pooled_records(idx, dense, weights).reshape(B, m.record_len))
        else:
            want = job.w0.gather_pooled_records(idx, dense, weights).reshape(B, m.record_len)
        for r in range(G):
            assert job.ctxs[r].pooled_index_cols == int(hots.sum())
            got, name = slice_bytes(fr, job.ctxs[r], job.wks[r], hots, idx, dense, None, weights, csr)
            got = got.view(np.uint32)
            assert got.shape == (B, F)
            assert np.array_equal(got[:, :lens[r]], want[:, offs[r]:offs[r] + lens[r]]), (r, fold)
            if kernel is not None:
                assert name == kernel, (name, kernel)


# ---- case 2: low-precision slices (GPU) ------------------------------------------------------------------------------------------------------
def lp_kernel_for(hots, aligned):
    """frk_gather_pooled's choice for a bf16 / e4m3 slice: the shape of the fp32 gather, or -- for the two shapes without those store arms -- its neighbour."""
    k = GM.pooled_kernel_for(hots, aligned)
    return {"gather_pooled_kernel<4, 2, false>": "gather_pooled_kernel<2, 2, false>", "gather_pooled_kernel<2, 4, false>": "gather_pooled_kernel<2, 8, false>"}.get(k, k)


def lp_expected(fr, f32_slice, transport, e_x):
    """The one-hot slice gather's rounding of an fp32 slice (uint32 [B][F]) -> uint8 [B][F * esz]."""
    x = f32_slice.view(np.float32)
    if transport == fr.FC_BF16:
        return np.ascontiguousarray((bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)).view(np.uint8)
    return e4m3_encode(np.clip(x.astype(np.float64) * 2.0 ** e_x, -448, 448))


def check_lp_slices(fr, device, pattern, fold="sum", shift=0, e_shift=0):
    """G = 3, batch 37 (the last chunk is part empty): fr_worker_gather_slices_pooled[_csr] in bf16 and e4m3 equals the documented rounding of the
    same context's fp32 slice, byte for byte over [0, slice_len) of every item, through the shape lp_kernel_for names; nothing behind the rows changes."""
    G, B = 3, 37
    m = model_c(fr, device)
    hots = cycle(pattern, m.idx_cols)
    modes = cycle((fr.POOL_SUM, fr.POOL_MEAN), m.idx_cols) if fold == "mean" else None
    offs, lens, F = m.shard_plan(G)
    rng = np.random.default_rng(2000 + len(pattern) + 7 * int(max(pattern)) + shift)
    with Job(fr, device, G, hots, modes, prec="fp8", whole=False, comms=False) as job:
        idx, dense, weights, csr = fold_inputs(job, rng, B, fold)
        kernel = lp_kernel_for(hots, aligned=shift == 0 and not csr)
        for r in range(G):
            ctx, wk = job.ctxs[r], job.wks[r]
            act, _ = ctx.fp8_exponents()
            act = [int(a) for a in act]
            act[0] += e_shift
            ctx.set_fp8_act_exponents(act)
            f32, name32 = slice_bytes(fr, ctx, wk, hots, idx, dense, fr.FC_FP32, weights, csr, shift)
            assert name32 == GM.pooled_kernel_for(hots, aligned=shift == 0 and not csr), name32
            f32 = f32.view(np.uint32)
            for tp in (fr.FC_BF16, fr.FC_FP8):
                esz = 2 if tp == fr.FC_BF16 else 1
                got, name = slice_bytes(fr, ctx, wk, hots, idx, dense, tp, weights, csr, shift)
                assert name == kernel, (name, kernel)
                want = lp_expected(fr, f32, tp, act[0])
                assert got.shape == want.shape == (B, F * esz)
                assert np.array_equal(got[:, :lens[r] * esz], want[:, :lens[r] * esz]), (r, tp, fold)


# ---- case 3: one live slot per bag equals one-hot ---------------------------------------------------------------------------------------------
def one_live_slot(rng, hots, ids):
    """int32 [B][P]: bag (b, c) holds ids[b][c] in one random slot, -1 in every other."""
    B = len(ids)
    pre = P.prefix_of(hots)
    idx = np.full((B, int(np.sum(hots))), -1, np.int32)
    for c, h in enumerate(hots):
        idx[np.arange(B), pre[c] + rng.integers(0, h, size=B)] = ids[:, c]
    return idx


def check_one_live_slot_equals_one_hot(fr, device, G, prec):
    """With exactly one non-empty slot per bag the fold is a bit copy of one row: the pooled slices equal fr_worker_gather_slices on those ids and
    the pooled step's scores equal fr_worker_submit_sharded's on the same contexts and communicators -- no tolerance, B = 301 and 5, both exchange modes."""
    m = model_c(fr, device)
    hots = cycle((1, 2, 3, 8), m.idx_cols)
    rng = np.random.default_rng(3000 + G)
    tp = precision(fr, prec)
    with Job(fr, device, G, hots, prec=prec, whole=False) as job:
        if prec == "fp8":
            ids_c = P.random_bags(rng, m.index_ranges(), np.ones(m.idx_cols, np.int32), 256)
            dense_c = job.dense(rng, 256)
            job.collective(lambda r: job.wks[r].calibrate_fp8_sharded(job.comms[r], ids_c, dense_c))
        for B in (301, 5):
            ids = P.random_bags(rng, m.index_ranges(), np.ones(m.idx_cols, np.int32), B)
            idx = one_live_slot(rng, hots, ids)
            dense = job.dense(rng, B)
            if device != CPU:
                F = job.ctxs[0].shard_info()["slice_padded"]
                esz = {"f32": 4, "bf16": 2, "fp8": 1}[prec]
                for r in (0, G - 1):
                    ctx, wk = job.ctxs[r], job.wks[r]
                    got, _ = slice_bytes(fr, ctx, wk, hots, idx, dense, tp)
                    d_i = fr.DeviceBuffer.from_numpy(ctx, ids)
                    d_d = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
                    d_s = fr.DeviceBuffer.from_numpy(ctx, np.full(B * F * esz, CANARY, np.uint8))
                    wk.gather_slices(B, d_i, d_d, d_s, tp)
                    wk.sync()
                    want = d_s.download(np.uint8, B * F * esz).reshape(B, F * esz)
                    n = m.shard_plan(G)[1][r] * esz
                    assert np.array_equal(got[:, :n], want[:, :n]), (G, prec, B, r)
            for mode in (fr.EXCHANGE_ALLGATHER, fr.EXCHANGE_ALLTOALL):
                job.set_exchange(mode)
                want = job.one_hot_step(ids, dense)
                got = job.pooled_step(idx, dense)
                assert np.array_equal(got, want), (G, prec, B, mode)
                assert np.array_equal(job.pooled_step(idx, dense, csr=True), want), (G, prec, B, mode)


# ---- case 4: real bags through the step ------------------------------------------------------------------------------------------------------
REAL_BAGS = (1, 2, 3, 5, 8, 16)      # mixed bag lengths


def host_fp8_exponents(rec_f32, ws, dims):
    """The library's calibration rule restated: activation exponents floor(log2(448 / (2 max|.|))) of the record and of every hidden activation of the
    fp32 chain (one binade of headroom), weight exponents floor(log2(448 / max|W|))."""
    x = rec_f32.astype(np.float64)
    act = []
    for l in range(4):
        act.append(int(np.floor(np.log2(448.0 / (2.0 * np.abs(x).max())))))
        if l < 3:
            x = (x @ ws[l].reshape(dims[l], dims[l + 1]).astype(np.float64)).astype(np.float32).astype(np.float64)
    return act, [int(np.floor(np.log2(448.0 / np.abs(ws[l]).max()))) for l in range(3)]


def real_bag_inputs(fr, m, fold, B):
    """The bags of case 4, by fold and batch alone (the CPU pre-check and the GPU step take the same)."""
    hots = cycle(REAL_BAGS, m.idx_cols)
    modes = cycle((fr.POOL_SUM, fr.POOL_MEAN), m.idx_cols) if fold == "mean" else None
    rng = np.random.default_rng(4000 + B + {"sum": 0, "mean": 1, "weighted": 2}[fold])
    idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.2, empty_bags=4)
    dense = P.dense_for(rng, m, B)
    weights = rng.uniform(0.25, 2.0, idx.shape).astype(np.float32) if fold == "weighted" else None
    return hots, modes, idx, dense, weights


def cpu_pooled_records(fr, m, hots, modes, idx, dense, weights):
    """Pooled fp32 records [B][K] from the CPU back-end, and the FC weights of the standard fill."""
    c = fr.Context(m, device=CPU)
    try:
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        c.set_pooling(hots, modes)
        wk = fr.Worker(c, len(idx))
        rec = wk.gather_pooled_records(idx, dense, weights).reshape(len(idx), m.record_len).view(np.float32)
        ws = [c.get_weights(l) for l in range(4)]
        wk.close()
        return rec, ws
    finally:
        c.close()


def fp32_chain(rec_f32, ws, dims):
    x = rec_f32.astype(np.float64)
    for l in range(3):
        x = x @ ws[l].reshape(dims[l], dims[l + 1]).astype(np.float64)
    return (x @ ws[3].astype(np.float64)).astype(np.float32)


def check_restatements_hold_on_the_chosen_bags(fr, device, fold, B):
    """Host only: on case 4's bags and seeds the bf16 and fp8 restatements themselves stay inside 3e-2 / 0.15 of the fp32 chain (with the calibration
    rule's exponents) -- otherwise no device could meet those bounds on them."""
    m = model_c(fr, device)
    hots, modes, idx, dense, weights = real_bag_inputs(fr, m, fold, B)
    rec, ws = cpu_pooled_records(fr, m, hots, modes, idx, dense, weights)
    dims = m.fc
    ref = fp32_chain(rec, ws, dims)
    e16 = rel_err(chain_bf16_reference(rec, ws, dims), ref)
    act, wexp = host_fp8_exponents(rec, ws, dims)
    e8 = rel_err(chain_fp8_reference(rec, ws, dims, act, wexp), ref)
    print("restatements vs fp32 chain, %s B=%d: bf16 %.3g fp8 %.3g" % (fold, B, e16, e8))
    assert e16 <= TOL["bf16"] and e8 <= TOL["fp8"], (e16, e8)


def check_real_bags(fr, device, G, prec, fold, B=301, csr=False):
    """Mixed bag lengths through fr_worker_submit_sharded_pooled: every rank ends with the same B scores; the offsets form's equal the padded form's;
    fp32 within 1e-5 of the unsharded fr_worker_submit_pooled*, bf16 / fp8 within 3e-2 / 0.15 of the host restatement on CPU-pooled records; the fp8
    exponents come from fr_worker_calibrate_fp8_sharded_pooled and are the same on every rank."""
    m = model_c(fr, device)
    hots, modes, idx, dense, weights = real_bag_inputs(fr, m, fold, B)
    dims = m.fc
    with Job(fr, device, G, hots, modes, prec=prec, whole=prec == "f32") as job:
        if prec == "fp8":
            job.collective(lambda r: job.wks[r].calibrate_fp8_sharded_pooled(job.comms[r], idx, dense, weights))
            exps = [c.fp8_exponents() for c in job.ctxs]
            assert all((list(e[0]), list(e[1])) == (list(exps[0][0]), list(exps[0][1])) for e in exps), exps
        got = job.pooled_step(idx, dense, weights)
        if csr:
            assert np.array_equal(job.pooled_step(idx, dense, weights, csr=True), got)
        if prec == "f32":
            err = rel_err(got, job.w0.infer_pooled(idx, dense, weights))
        else:
            rec, ws = cpu_pooled_records(fr, m, hots, modes, idx, dense, weights)
            if prec == "bf16":
                ref = chain_bf16_reference(rec, ws, dims)
            else:
                act, wexp = job.ctxs[0].fp8_exponents()
                ref = chain_fp8_reference(rec, ws, dims, [int(a) for a in act], [int(w) for w in wexp])
            err = rel_err(got, ref)
        print("pooled step G=%d %s %s B=%d: rel err %.3g (bound %g)" % (G, prec, fold, B, err, TOL[prec]))
        assert err <= TOL[prec], (G, prec, fold, err)


# ---- case 5: calibration sees the bags (GPU) -------------------------------------------------------------------------------------------------
def check_calibration_sees_the_bags(fr, device):
    """16-slot SUM bags: act_exp[0] of the pooled calibration is strictly below the one-hot calibration's on the same contexts, and with it no
    element of the e4m3 slice is +-448."""
    G, B = 2, 301
    m = model_c(fr, device)
    hots = np.full(m.idx_cols, 16, np.int32)
    rng = np.random.default_rng(5000)
    with Job(fr, device, G, hots, prec="fp8", whole=False) as job:
        ids = P.random_bags(rng, m.index_ranges(), np.ones(m.idx_cols, np.int32), B)
        idx = job.bags(rng, B, empty_share=0.0, empty_bags=0)
        dense = job.dense(rng, B)
        job.collective(lambda r: job.wks[r].calibrate_fp8_sharded(job.comms[r], ids, dense))
        one_hot = [int(c.fp8_exponents()[0][0]) for c in job.ctxs]
        job.collective(lambda r: job.wks[r].calibrate_fp8_sharded_pooled(job.comms[r], idx, dense))
        pooled = [int(c.fp8_exponents()[0][0]) for c in job.ctxs]
        assert len(set(one_hot)) == 1 and len(set(pooled)) == 1, (one_hot, pooled)
        assert pooled[0] < one_hot[0], (pooled, one_hot)
        lens = m.shard_plan(G)[1]
        for r in range(G):
            got, _ = slice_bytes(fr, job.ctxs[r], job.wks[r], hots, idx[:37], None if dense is None else dense[:37], fr.FC_FP8)
            assert not np.isin(got[:, :lens[r]], (0x7E, 0xFE)).any(), r


# ---- case 6: errors and state ----------------------------------------------------------------------------------------------------------------
def owned_column(fr, m, G, q):
    """An index column (PER_TABLE: a table) with a TABLE segment inside rank q's slice."""
    offs, lens, _ = m.shard_plan(G)
    return [s.src for s in m.segments() if s.kind == P.SEG_TABLE and offs[q] <= s.rec_offset < offs[q] + lens[q]][0]


def check_errors_reach_the_owning_ranks(fr, device, G=3, q=1):
    """An out-of-range id and a malformed bag in a column owned by rank q: rank by rank the status fr_worker_sync gives for the one-hot step with an
    out-of-range id in the same column; every rank's step completes, and the workers are usable afterwards."""
    m = model_c(fr, device)
    hots = cycle((2, 3, 4), m.idx_cols)
    pre = P.prefix_of(hots)
    rng = np.random.default_rng(6000 + G)
    B = 37
    col = owned_column(fr, m, G, q)
    rows = int(m.index_ranges()[col])
    with Job(fr, device, G, hots, whole=False) as job:
        ids = P.random_bags(rng, m.index_ranges(), np.ones(m.idx_cols, np.int32), B)
        idx = job.bags(rng, B, empty_share=0.0, empty_bags=0)
        dense = job.dense(rng, B)
        good = job.pooled_step(idx, dense)
        bad_ids = ids.copy()
        bad_ids[7, col] = rows

        def load_one_hot(wk):
            wk.idx[:B] = bad_ids
            if wk.dense is not None:
                wk.dense[:B] = dense
        want, _ = job.statuses(B, load_one_hot, lambda wk, cm: wk.submit_sharded(cm, B))
        assert want[q] == fr.FR_ERR_INDEX_RANGE and fr.FR_OK in want, want
        # an out-of-range id in a slot of the column's bag, padded form and offsets form
        bad = idx.copy()
        bad[7, pre[col] + 1] = rows
        st, _ = job.statuses(B, lambda wk: wk.load_pooled(bad, dense), lambda wk, cm: wk.submit_sharded_pooled(cm, B))
        assert st == want, (st, want)
        off, ind, _ = fr.bags_to_csr(bad, hots)
        st, _ = job.statuses(B, lambda wk: wk.load_pooled_csr(off, ind, dense), lambda wk, cm: wk.submit_sharded_pooled_csr(cm, B))
        assert st == want, (st, want)
        assert np.array_equal(job.pooled_step(idx, dense), good)
        # a malformed bag: bag (7, col) one entry longer than the column's cap (an entry of item 0 is dropped, so that nnz stays within batch x P)
        fewer = idx.copy()
        fewer[0, 0] = -1
        off, ind, _ = fr.bags_to_csr(fewer, hots)
        at = int(off[7 * m.idx_cols + col + 1])
        ind = np.insert(ind, at, 0).astype(np.int32)
        off = off.copy()
        off[7 * m.idx_cols + col + 1:] += 1
        st, _ = job.statuses(B, lambda wk: wk.load_pooled_csr(off, ind, dense), lambda wk, cm: wk.submit_sharded_pooled_csr(cm, B))
        assert st == want, (st, want)
        assert np.array_equal(job.pooled_step(idx, dense), good)          # every worker is usable afterwards
        assert np.array_equal(job.pooled_step(idx, dense, csr=True), good)


def check_state_and_arguments(fr, device, G=2):
    """Kind (1) returns (nothing enqueued, the communicator stays usable), the creation-time contract, and creation's argument errors."""
    L = fr.lib()
    m = model_c(fr, device)
    cols = m.idx_cols
    hots = cycle((2, 3), cols)
    rng = np.random.default_rng(6100)
    B = 37
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    # creation: mismatched n_cols, bad hots, a bad mode -> FR_ERR_INVALID and no context
    for h, md, n in ((hots, None, cols + 1), (hots[:-1], None, cols - 1), (np.where(np.arange(cols) == 1, 0, hots).astype(np.int32), None, cols),
                     (np.where(np.arange(cols) == 1, fr.POOL_MAX_HOTS + 1, hots).astype(np.int32), None, cols), (hots, np.full(cols, 2, np.int32), cols)):
        out = ctypes.c_void_p()
        rc = L.fr_ctx_create_sharded_pooled(m._ptr, device, 0, G, pi(np.ascontiguousarray(h)), pi(md) if md is not None else None, n, ctypes.byref(out))
        assert rc == fr.FR_ERR_INVALID and not out.value, (rc, out.value, n)
    # a sharded context created WITHOUT pooling: the pooled step is a state error, and the one-hot step still runs on the same communicators
    with Job(fr, device, G, None, whole=False) as job:
        ids = P.random_bags(rng, m.index_ranges(), np.ones(cols, np.int32), B)
        dense = job.dense(rng, B)
        before = job.one_hot_step(ids, dense)
        for r in range(G):
            assert L.fr_worker_submit_sharded_pooled(job.wks[r]._h, job.comms[r]._h, B, 0) == fr.FR_ERR_STATE
            assert L.fr_worker_submit_sharded_pooled_csr(job.wks[r]._h, job.comms[r]._h, B, 0) == fr.FR_ERR_STATE
            assert L.fr_ctx_set_pooling(job.ctxs[r]._h, pi(hots), cols) == fr.FR_ERR_STATE and job.ctxs[r].pooled_index_cols == 0
        assert np.array_equal(job.one_hot_step(ids, dense), before)
    # created with pooling (one MEAN column): set_pooling[_modes] are refused and change nothing; weights with a MEAN column are a state error
    modes = np.where(np.arange(cols) == 0, fr.POOL_MEAN, fr.POOL_SUM).astype(np.int32)
    with Job(fr, device, G, hots, modes, whole=False) as job:
        idx = job.bags(rng, B)
        dense = job.dense(rng, B)
        good = job.pooled_step(idx, dense)
        for r in range(G):
            c = job.ctxs[r]
            assert L.fr_ctx_set_pooling(c._h, pi(np.ones(cols, np.int32)), cols) == fr.FR_ERR_STATE
            assert L.fr_ctx_set_pooling(c._h, None, 0) == fr.FR_ERR_STATE
            assert L.fr_ctx_set_pooling_modes(c._h, None, 0) == fr.FR_ERR_STATE
            assert c.pooled_index_cols == int(hots.sum()) and np.array_equal(c.pooling_modes, modes)
            assert L.fr_worker_submit_sharded_pooled(job.wks[r]._h, job.comms[r]._h, B, 1) == fr.FR_ERR_STATE
            assert L.fr_worker_submit_sharded_pooled_csr(job.wks[r]._h, job.comms[r]._h, B, 1) == fr.FR_ERR_STATE
            assert L.fr_worker_submit_pooled(job.wks[r]._h, B) == fr.FR_ERR_STATE            # a shard cannot run the chain alone
            job.wks[r].sync()                                                                  # ... and nothing was enqueued
            # the offsets form's host checks, before anything is enqueued
            job.wks[r].pool_offsets[0] = 1
            assert L.fr_worker_submit_sharded_pooled_csr(job.wks[r]._h, job.comms[r]._h, B, 0) == fr.FR_ERR_INVALID
            job.wks[r].pool_offsets[0] = 0
            job.wks[r].pool_offsets[B * cols] = B * int(hots.sum()) + 1
            assert L.fr_worker_submit_sharded_pooled_csr(job.wks[r]._h, job.comms[r]._h, B, 0) == fr.FR_ERR_INVALID
        assert np.array_equal(job.pooled_step(idx, dense), good)
        if device == CPU:      # the CPU back-end gathers fp32 only: the one-hot call's refusal
            off = fr.DeviceBuffer(job.ctxs[0], B * job.ctxs[0].shard_info()["slice_padded"] * 4)
            with pytest.raises(fr.FleetRecError) as e:
                job.wks[0].gather_slices_pooled(B, fr.DeviceBuffer.from_numpy(job.ctxs[0], idx), fr.DeviceBuffer.from_numpy(job.ctxs[0], dense), off, fr.FC_BF16)
            assert e.value.status == fr.FR_ERR_STATE and "fp32 records only" in str(e.value)
    # n_shards == 1: a plain context with pooling set
    c1 = fr.Context(m, device=device, shard_rank=0, n_shards=1, hots=hots)
    try:
        assert c1.pooled_index_cols == int(hots.sum())
        c1.set_pooling(np.ones(cols, np.int32))
        assert c1.pooled_index_cols == cols
    finally:
        c1.close()


# ---- case 7: the failure protocol under the pooled step (GPU) --------------------------------------------------------------------------------
def check_fc_failure_reaches_every_rank(fr, device, G=3):
    """The assertion block of the staged one-hot test, through fr_worker_submit_sharded_pooled: an injected FC failure on rank q -> every rank's sync
    names q, q's items are NaN, the rest are right."""
    m = model_c(fr, device)
    hots = cycle((1, 2, 3, 8), m.idx_cols)
    rng = np.random.default_rng(7000)
    B, q = 301, G - 1
    with Job(fr, device, G, hots, whole=False) as job:
        idx = job.bags(rng, B)
        dense = job.dense(rng, B)
        good = job.pooled_step(idx, dense)
        job.wks[q].inject_fc_failure(1)
        for r in range(G):
            job.wks[r].load_pooled(idx, dense)
            job.wks[r].submit_sharded_pooled(job.comms[r], B)
        base, rem = B // G, B % G
        lo = q * base + min(q, rem)
        hi = lo + base + (1 if q < rem else 0)
        for r in range(G):
            with pytest.raises(fr.FleetRecError) as e:
                job.wks[r].sync()
            assert e.value.status == fr.FR_ERR_COMM and "shard rank %d reported a failed FC chain" % q in str(e.value), (r, str(e.value))
            sc = job.wks[r].score[:B]
            assert np.isnan(sc[lo:hi]).all() and np.array_equal(sc[:lo], good[:lo]) and np.array_equal(sc[hi:], good[hi:]), r
        assert np.array_equal(job.pooled_step(idx, dense), good)          # nothing was aborted

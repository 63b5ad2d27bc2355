"""GPU tests of the all-to-all exchange mode of the table-sharded step (fr_comm_set_exchange, include/fleetrec.h): G shard contexts on the one
GPU of a test box through the staged host exchange, a one-rank RCCL communicator (ncclSend / ncclRecv to itself), full-size configs[3], and a
two-GPU RCCL case where two GPUs are visible.  In every precision the all-to-all step must give the all-gather step's scores bit for bit:
the same gather, transpose and FC kernels read the same elements, only fewer of them travel."""
import threading

import numpy as np
import pytest
from gpu_helpers import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

PRECS = {"f32": 0, "bf16": 1, "fp8": 2}
ESZ = {"f32": 4, "bf16": 2, "fp8": 1}


def item_range(r, G, B):
    base, rem = divmod(B, G)
    lo = r * base + min(r, rem)
    return lo, base + (1 if r < rem else 0)


def shard_job(fr, gpu, m, G, prec, max_batch):
    ctxs_, wks = [], []
    for r in range(G):
        c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        c.set_fc_precision(PRECS[prec])
        ctxs_.append(c)
        wks.append(fr.Worker(c, max_batch))
    return ctxs_, wks


def close_all(wks, comms, ctxs_):
    for w in wks:
        w.close()
    for cm in comms:
        cm.close()
    for c in ctxs_:
        c.close()


def step(wks, comms, idx, dense):
    """One sharded step, submitted on every rank from one thread, then synchronised -> every rank's scores."""
    B = len(idx)
    for w in wks:
        w.idx[:B] = idx
        w.dense[:B] = dense
    for r in range(len(wks)):
        wks[r].submit_sharded(comms[r], B)
    got = []
    for r in range(len(wks)):
        wks[r].sync()
        got.append(wks[r].score[:B].copy())
    return got


def calibrate(wks, comms, idx, dense):
    """The sharded fp8 calibration is a synchronous collective: one thread per rank."""
    th = [threading.Thread(target=lambda r=r: wks[r].calibrate_fp8_sharded(comms[r], idx, dense)) for r in range(len(wks))]
    [t.start() for t in th]
    [t.join(300) for t in th]
    assert not any(t.is_alive() for t in th)


def check_bytes(comms, G, B, P, esz, alltoall):
    for r, cm in enumerate(comms):
        _, n_r = item_range(r, G, B)
        want = ((G - 1) * n_r * P * esz, (B - n_r) * P * esz) if alltoall else ((G - 1) * B * P * esz, (G - 1) * B * P * esz)
        assert cm.exchange_bytes() == want, (G, B, r, cm.exchange_bytes(), want)


@pytest.mark.parametrize("G", [2, 3, 8])
@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_staged_alltoall_bit_identical_to_allgather(fr, gpu, G, prec):
    """G ranks on one GPU (the staged exchange: D2H of the slice, host all-to-all, H2D of only G * n_r rows), row-capped Model-C, B = 301
    and a batch smaller than G: every rank's scores in all-to-all mode equal the all-gather mode's on the same contexts, bit for bit; the
    byte counters follow fleetrec_diag.h.  fp8: one sharded calibration before both modes."""
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=20000)
    _, _, P = m.shard_plan(G)
    ctxs_, wks = shard_job(fr, gpu, m, G, prec, 512)
    comms = []
    rng = np.random.default_rng(700 + G)
    try:
        comms = fr.Comm.init_all(ctxs_)
        if prec == "fp8":
            idx_c = uniform_idx(rng, m.rows(), 512)
            calibrate(wks, comms, idx_c, rng.uniform(-1, 1, (512, m.dense_len)).astype(np.float32))
            assert all(c.fp8_exponents() == ctxs_[0].fp8_exponents() for c in ctxs_)
        for B in (301, G - 1):
            idx = uniform_idx(rng, m.rows(), B)
            dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
            for cm in comms:
                cm.set_exchange("allgather")
            ag = step(wks, comms, idx, dense)
            check_bytes(comms, G, B, P, ESZ[prec], False)
            for cm in comms:
                cm.set_exchange("alltoall")
            a2a = step(wks, comms, idx, dense)
            check_bytes(comms, G, B, P, ESZ[prec], True)
            for r in range(G):
                assert np.array_equal(ag[r], ag[0]) and np.array_equal(a2a[r], ag[0]), (G, prec, B, r)
            assert np.isfinite(ag[0]).all()
    finally:
        close_all(wks, comms, ctxs_)


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_alltoall_through_rccl_one_rank(fr, gpu, prec):
    """A one-rank RCCL communicator through the unique-id path: the all-to-all is a grouped ncclSend / ncclRecv of the rank to itself.
    Scores in all-to-all mode equal the all-gather mode's bit for bit, and the unsharded submit's (fp32: within 1e-5, the split-K order of
    the unsharded chain; bf16 / fp8: bit for bit, as test_gpu_sharded.py checks for the all-gather)."""
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=30000)
    ctx = fr.Context(m, device=gpu, shard_rank=0, n_shards=1)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    ctx.set_fc_precision(PRECS[prec])
    comm = fr.Comm.init_rank(ctx, fr.Comm.unique_id())
    wk = fr.Worker(ctx, 512)
    try:
        comm.set_wait_ms(20000)
        rng = np.random.default_rng(41)
        B = 300
        idx = uniform_idx(rng, m.rows(), B)
        dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
        if prec == "fp8":
            wk.calibrate_fp8_sharded(comm, idx, dense)
        ag = wk.infer_sharded(comm, idx, dense)
        assert comm.exchange_bytes() == (0, 0)             # one rank: no peer bytes
        comm.set_exchange("alltoall")
        assert comm.exchange == fr.EXCHANGE_ALLTOALL
        a2a = wk.infer_sharded(comm, idx, dense)
        assert np.array_equal(a2a, ag)
        assert np.array_equal(wk.infer_sharded(comm, idx[:77], dense[:77]), a2a[:77]) if prec != "f32" else True
        plain = wk.infer(idx, dense)
        assert np.array_equal(a2a, plain) if prec != "f32" else rel_err(a2a, plain) <= 1e-5
    finally:
        wk.close()
        comm.close()
        ctx.close()


def test_staged_alltoall_fc_failure_names_the_rank(fr, gpu):
    """Failure protocol kind (2) under the all-to-all mode, on the device: an injected FC failure on rank q of a staged G = 3 job makes every
    rank's sync return FR_ERR_COMM naming q; q's items are NaN on every rank, the others equal a good step's."""
    G, B, q = 3, 301, 1
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=20000)
    ctxs_, wks = shard_job(fr, gpu, m, G, "bf16", 512)
    comms = []
    rng = np.random.default_rng(77)
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    try:
        comms = fr.Comm.init_all(ctxs_)
        for cm in comms:
            cm.set_exchange("alltoall")
        good = step(wks, comms, idx, dense)[0]
        wks[q].inject_fc_failure(1)
        for r in range(G):
            wks[r].submit_sharded(comms[r], B)
        lo, n = item_range(q, G, B)
        for r in range(G):
            with pytest.raises(fr.FleetRecError) as e:
                wks[r].sync()
            assert e.value.status == fr.FR_ERR_COMM and "shard rank %d reported a failed FC chain" % q in str(e.value), (r, str(e.value))
            sc = wks[r].score[:B]
            assert np.isnan(sc[lo:lo + n]).all() and np.array_equal(sc[:lo], good[:lo]) and np.array_equal(sc[lo + n:], good[lo + n:]), r
        assert all(np.array_equal(g, good) for g in step(wks, comms, idx, dense))   # the communicator survived
    finally:
        close_all(wks, comms, ctxs_)


def test_config3_full_size_eight_ranks_alltoall(fr, gpu):
    """BASELINE configs[3] through the C-ABI step in all-to-all mode: FULL-size Model-C (63.2 GB of tables in eight shard contexts on the
    one GPU, the staged exchange), batch 4096, bf16: every rank's scores equal the all-gather step's on the same contexts, bit for bit."""
    G, B = 8, 4096
    m = fr.Model.builtin(fr.MODEL_C)
    _, _, P = m.shard_plan(G)
    ctxs_, wks, comms = [], [], []
    rng = np.random.default_rng(4097)
    idx = uniform_idx(rng, m.rows(), B)
    idx[0], idx[1] = 0, m.rows() - 1
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    try:
        ctxs_, wks = shard_job(fr, gpu, m, G, "bf16", B)
        comms = fr.Comm.init_all(ctxs_)
        ag = step(wks, comms, idx, dense)
        for cm in comms:
            cm.set_exchange("alltoall")
        a2a = step(wks, comms, idx, dense)
        check_bytes(comms, G, B, P, 2, True)
        for r in range(G):
            assert np.array_equal(ag[r], ag[0]) and np.array_equal(a2a[r], ag[0]), r
        assert np.isfinite(ag[0]).all()
    finally:
        close_all(wks, comms, ctxs_)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_alltoall_through_rccl_two_ranks(fr, gpu, prec):
    """G = 2 over RCCL on two devices (grouped ncclSend / ncclRecv with uneven counts: B = 301 -> 151 + 150 items): the all-to-all step gives
    the all-gather step's scores bit for bit on every rank.  Skipped where fewer than two GPUs are visible."""
    if fr.device_count() < 2:
        pytest.skip("needs two GPUs: the G > 1 RCCL path is unmeasured on one-GPU boxes")
    G, B = 2, 301
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=30000)
    _, _, P = m.shard_plan(G)
    ctxs_, wks, comms = [], [], []
    for r in range(G):
        c = fr.Context(m, device=r, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        c.set_fc_precision(PRECS[prec])
        ctxs_.append(c)
        wks.append(fr.Worker(c, 512))
    rng = np.random.default_rng(33)
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    try:
        comms = fr.Comm.init_all(ctxs_)
        for cm in comms:
            cm.set_wait_ms(20000)
        out = {}
        for mode in ("allgather", "alltoall"):
            for cm in comms:
                cm.set_exchange(mode)
            got, errs = [None] * G, [None] * G

            def run(r):
                try:
                    got[r] = wks[r].infer_sharded(comms[r], idx, dense)
                except Exception as ex:   # noqa: BLE001
                    errs[r] = ex
            th = [threading.Thread(target=run, args=(r,)) for r in range(G)]
            [t.start() for t in th]
            [t.join(120) for t in th]
            assert not any(t.is_alive() for t in th) and errs == [None, None], errs
            out[mode] = got
        check_bytes(comms, G, B, P, ESZ[prec], True)
        for r in range(G):
            assert np.array_equal(out["alltoall"][r], out["allgather"][0]), r
    finally:
        close_all(wks, comms, ctxs_)

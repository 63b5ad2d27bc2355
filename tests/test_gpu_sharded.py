"""GPU parity, part 4: table-sharded contexts (configs[3] / configs[4]) in single-GPU emulation and through RCCL with the ranks one GPU offers.
Tolerances, seeds and reference chains: tests/gpu_helpers.py; the full-size contexts (`ctxs`): tests/conftest.py."""
import os
import threading

import numpy as np
import pytest
from gpu_helpers import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("which,G", [(0, 2), (1, 4), (2, 8), (2, 70)])   # 70 shards: the slice transposes take 64 shards per launch
def test_table_sharded_mode_single_device_emulation(fr, O, gpu, which, G):
    """BASELINE config 4 on one GPU: G table-sharded contexts (each holds only its tables), every shard gathers its
    [B x F] slice, the all-gather is emulated by concatenating the slices in shard order, then 'rank' r runs the FC chain on
    its B/G items from the gathered layout.  Must equal the oracle (records bit-exact, scores 1e-3) and the unsharded path."""
    import importlib
    dist_mod = importlib.import_module("fleetrec_amd.dist")
    m = fr.Model.builtin(which).clone(max_rows=20000)
    om = O.OracleModel(NAMES[which])
    offs, lens, F = m.shard_plan(G)
    rng = np.random.default_rng(100 + G)
    B = 200
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32) if m.dense_len else None
    full = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES)
    ctxs_, slices = [], []
    for r in range(G):
        c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
        info = c.shard_info()
        assert (info["slice_offset"], info["slice_len"], info["slice_padded"]) == (offs[r], lens[r], F)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        wk = fr.Worker(c, B)
        sl = wk.gather_records(idx, dense).reshape(B, F)
        assert np.array_equal(sl[:, :lens[r]], full[:, offs[r]:offs[r] + lens[r]])   # the shard's slice, bit-exact
        with pytest.raises(fr.FleetRecError):                                         # a shard cannot run the whole path alone
            wk.submit_device(B, None, None, None)
        ctxs_.append((c, wk))
        slices.append(sl)
    gathered = np.stack(slices)                                                       # == ncclAllGather of the G slices
    assert np.array_equal(dist_mod.assemble_records(gathered, offs, lens, m.record_len), full)
    ws = [ctxs_[0][0].get_weights(l) for l in range(4)]
    ref = om.fc_chain(full.view(np.float32), ws, acc64=True)
    scores = np.empty(B, np.float32)
    for r, (c, wk) in enumerate(ctxs_):
        lo, hi = dist_mod.item_range(r, G, B)
        d_g = fr.DeviceBuffer.from_numpy(c, gathered)
        d_s = fr.DeviceBuffer(c, max(hi - lo, 1) * 4)
        wk.fc_from_slices(B, lo, hi - lo, d_g, d_s)
        wk.sync()
        scores[lo:hi] = d_s.download(np.float32, hi - lo)
    assert rel_err(scores, ref) <= 1e-3
    # all-to-all variant (section 8(f) N2): a rank only receives ITS items' slices -> [G][hi-lo][F]; same scores bit for bit
    for r, (c, wk) in enumerate(ctxs_):
        lo, hi = dist_mod.item_range(r, G, B)
        mine = np.ascontiguousarray(gathered[:, lo:hi, :])
        d_g = fr.DeviceBuffer.from_numpy(c, mine)
        d_s = fr.DeviceBuffer(c, max(hi - lo, 1) * 4)
        wk.fc_from_slices(hi - lo, 0, hi - lo, d_g, d_s)
        wk.sync()
        assert np.array_equal(d_s.download(np.float32, hi - lo), scores[lo:hi])
    # unsharded context on the same inputs: same records, scores equal up to the split-K order of a different batch size
    c0 = fr.Context(m, device=gpu)
    c0.fill_tables(fr.FILL_HASH, SEED_TABLES)
    c0.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    w0 = fr.Worker(c0, B)
    assert np.abs(w0.infer(idx, dense) - scores).max() <= 1e-5 * np.abs(ref).max()
    w0.close()
    # BASELINE configs[4]: the sharded FC in the low-precision chains -- the all-gathered fp32 slices are re-packed to bf16 / e4m3
    # operands on the way into the chain; fp8 activation exponents come from a calibration on the gathered slices.  Same scores as
    # the unsharded context in the same precision, bit for bit (same operand images, same per-item arithmetic).
    for prec, tol32 in ((fr.FC_BF16, 3e-2), (fr.FC_FP8, 0.15)):
        lp = np.empty(B, np.float32)
        for r, (c, wk) in enumerate(ctxs_):
            c.set_fc_precision(prec)
            lo, hi = dist_mod.item_range(r, G, B)
            d_g = fr.DeviceBuffer.from_numpy(c, gathered)
            if prec == fr.FC_FP8:
                wk.calibrate_fp8_slices(B, 0, B, d_g)
            d_s = fr.DeviceBuffer(c, max(hi - lo, 1) * 4)
            wk.fc_from_slices(B, lo, hi - lo, d_g, d_s)
            wk.sync()
            lp[lo:hi] = d_s.download(np.float32, hi - lo)
        assert rel_err(lp, ref) <= tol32, (prec, rel_err(lp, ref))
        # low-precision TRANSPORT: the shards emit bf16 / e4m3 slices (half / a quarter of the all-gather bytes); they are exactly the
        # values the chain made of the fp32 slices above, so the scores do not change by a bit
        esz, dt = (2, np.uint16) if prec == fr.FC_BF16 else (1, np.uint8)
        lp_slices = []
        d_i = None
        for r, (c, wk) in enumerate(ctxs_):
            d_i = fr.DeviceBuffer.from_numpy(c, idx)
            d_d = fr.DeviceBuffer.from_numpy(c, dense) if dense is not None else None
            d_sl = fr.DeviceBuffer(c, B * F * esz)
            wk.gather_slices(B, d_i, d_d, d_sl, prec)
            wk.sync()
            lp_slices.append(d_sl.download(dt, B * F).reshape(B, F))
        if prec == fr.FC_BF16:   # the wire format itself: RNE of the fp32 slice
            for r in range(G):
                want16 = (bf16_round(slices[r].view(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
                assert np.array_equal(lp_slices[r][:, :lens[r]], want16[:, :lens[r]])
        g_lp = np.stack(lp_slices)
        tr = np.empty(B, np.float32)
        for r, (c, wk) in enumerate(ctxs_):
            lo, hi = dist_mod.item_range(r, G, B)
            d_g = fr.DeviceBuffer.from_numpy(c, g_lp)
            d_s = fr.DeviceBuffer(c, max(hi - lo, 1) * 4)
            wk.fc_from_slices_lp(B, lo, hi - lo, d_g, prec, d_s)
            wk.sync()
            tr[lo:hi] = d_s.download(np.float32, hi - lo)
        assert np.array_equal(tr, lp), prec
        with pytest.raises(fr.FleetRecError):   # the transport type must be the chain's precision
            ctxs_[0][1].fc_from_slices_lp(B, 0, 1, d_g, fr.FC_BF16 if prec == fr.FC_FP8 else fr.FC_FP8, d_s)
        c0.set_fc_precision(prec)
        w0 = fr.Worker(c0, B)
        if prec == fr.FC_FP8:
            w0.calibrate_fp8(idx, dense)
            assert c0.fp8_exponents() == ctxs_[0][0].fp8_exponents()
        assert np.array_equal(w0.infer(idx, dense), lp), prec
        w0.close()
    for c, wk in ctxs_:
        wk.close()
        c.close()
    c0.close()


def test_table_sharded_full_size_g8(fr, O, gpu):
    """BASELINE configs[3] at FULL table size AND full batch: Model-C's eight table-ID shards (63.2 GB together) side by side on one GPU,
    batch 4096 (the configuration's own batch), uniform indices over every table's whole row range.  Every shard's slice bit-exact against the oracle; every item's
    score (each computed by the shard that owns it, from the all-gathered layout) within 1e-3 of the fp64-accumulating oracle."""
    import importlib
    dist_mod = importlib.import_module("fleetrec_amd.dist")
    G, B = 8, 4096
    m = fr.Model.builtin(fr.MODEL_C)
    om = O.OracleModel("C")
    offs, lens, F = m.shard_plan(G)
    rng = np.random.default_rng(808)
    idx = uniform_idx(rng, m.rows(), B)
    idx[0], idx[1] = 0, m.rows() - 1
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    full = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES)
    shards, slices = [], []
    for r in range(G):
        c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        wk = fr.Worker(c, B)
        sl = wk.gather_records(idx, dense).reshape(B, F)
        assert np.array_equal(sl[:, :lens[r]], full[:, offs[r]:offs[r] + lens[r]]), r
        shards.append((c, wk))
        slices.append(sl)
    gathered = np.stack(slices)
    ws = [shards[0][0].get_weights(l) for l in range(4)]
    ref = om.fc_chain(full.view(np.float32), ws, acc64=True)
    scores = np.empty(B, np.float32)
    for r, (c, wk) in enumerate(shards):
        lo, hi = dist_mod.item_range(r, G, B)
        d_g = fr.DeviceBuffer.from_numpy(c, gathered)
        d_s = fr.DeviceBuffer(c, (hi - lo) * 4)
        wk.fc_from_slices(B, lo, hi - lo, d_g, d_s)
        wk.sync()
        scores[lo:hi] = d_s.download(np.float32, hi - lo)
        d_g.free()
        d_s.free()
    assert rel_err(scores, ref) <= 1e-3
    for c, wk in shards:
        wk.close()
        c.close()


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_submit_sharded_through_rccl_one_rank(fr, O, gpu, prec):
    """The sharded hot-loop body behind the C-ABI (fr_comm_* + fr_worker_submit_sharded) on the one GPU a test box has: a one-rank RCCL
    communicator (ncclCommInitRank through the unique-id path), so the all-gathers are degenerate but every call -- dlopen of
    librccl, communicator set-up, two ncclAllGather on the worker's stream, the slice transport formats -- really runs.  Scores must
    equal the unsharded submit of the same context geometry bit for bit (one shard = the whole record), the oracle within tolerance."""
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=30000)
    om = O.OracleModel("C")
    P = {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[prec]
    ctx = fr.Context(m, device=gpu, shard_rank=0, n_shards=1)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    ctx.set_fc_precision(P)
    comm = fr.Comm.init_rank(ctx, fr.Comm.unique_id())
    comm.set_wait_ms(20000)                            # the bound of fr_worker_sync's wait for the step's collectives (default 60 s)
    with pytest.raises(fr.FleetRecError):
        comm.set_wait_ms(0)
    rng = np.random.default_rng(31)
    B = 300
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    wk = fr.Worker(ctx, 512)
    if prec == "fp8":
        wk.calibrate_fp8_sharded(comm, idx, dense)
    got = wk.infer_sharded(comm, idx, dense)
    plain = wk.infer(idx, dense)                      # same context, unsharded path
    assert np.array_equal(got, plain) if prec != "f32" else rel_err(got, plain) <= 1e-5
    rec = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES).view(np.float32)
    ref = om.fc_chain(rec, [ctx.get_weights(l) for l in range(4)], acc64=True)
    assert rel_err(got, ref) <= {"f32": 1e-3, "bf16": 3e-2, "fp8": 0.15}[prec]
    again = wk.infer_sharded(comm, idx[:77], dense[:77])   # ragged batch, reuse: the step's own first result (fp32: another batch may sum in another order)
    assert np.array_equal(again, got[:77]) if prec != "f32" else rel_err(again, got[:77]) <= 1e-5
    # a communicator belongs to its context
    other = fr.Context(m, device=gpu)
    w2 = fr.Worker(other, 64)
    with pytest.raises(fr.FleetRecError):
        w2.infer_sharded(comm, idx[:8], dense[:8])
    w2.close()
    other.close()
    # fr_comm_destroy between a submit and its sync used to leave the worker with a dangling communicator; now the step in flight
    # keeps it alive and the sync completes normally
    wk.idx[:B] = idx
    wk.dense[:B] = dense
    fr._check(fr.lib().fr_worker_submit_sharded(wk._h, comm._h, B))
    comm.close()
    wk.sync()
    assert np.array_equal(wk.score[:B], got)
    wk.close()
    ctx.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_submit_sharded_through_rccl_full_size_batch_4096(fr, O, ctxs, prec):
    """The RCCL hot-loop body (fr_worker_submit_sharded: H2D -> slice gather in the chain's operand type -> ncclAllGather -> FC chain ->
    ncclAllGather of the scores and status words -> D2H) at the configuration's own size: FULL-size Model-C (63.2 GB), batch 4096 -- on the
    one-rank communicator a one-GPU box allows (VERDICT r04 missing 1: it had only run on row-capped tables at batch 300).  One shard = the
    whole record, so the scores must equal the unsharded submit of the same context bit for bit; 1024 of them against the oracle."""
    m, ctx = ctxs(2)
    om = O.OracleModel("C")
    P = {"bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[prec]
    B = 4096
    rng = np.random.default_rng(409 + P)
    idx = uniform_idx(rng, m.rows(), B)
    idx[0], idx[1] = 0, m.rows() - 1
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    ctx.set_fc_precision(P)
    try:
        comm = fr.Comm.init_rank(ctx, fr.Comm.unique_id())
        wk = fr.Worker(ctx, B)
        if prec == "fp8":
            wk.calibrate_fp8_sharded(comm, idx, dense)
        got = wk.infer_sharded(comm, idx, dense)
        assert np.array_equal(got, wk.infer(idx, dense))
        assert np.array_equal(wk.infer_sharded(comm, idx, dense), got)         # the step is repeatable on the same communicator
        sub = slice(1024, 2048)
        rec = om.gather(idx[sub], dense=dense[sub], content_mode=O.FILL_HASH, seed=SEED_TABLES).view(np.float32)
        ref = om.fc_chain(rec, [ctx.get_weights(l) for l in range(4)], acc64=True)
        assert np.abs(got[sub] - ref).max() <= {"bf16": 3e-2, "fp8": 0.15}[prec] * np.abs(ref).max()
        wk.close()
        comm.close()
    finally:
        ctx.set_chain_width(0)
        ctx.set_fc_precision(fr.FC_FP32)


def test_sharded_fc_failure_reaches_every_rank_through_the_status_word(fr, gpu):
    """a rank whose FC chain fails inside fr_worker_submit_sharded used to return its error locally while the peers completed
    the score all-gather with FR_OK and copied that rank's stale chunk.  Now the chunk travels as NaN and the rank's status word (one
    float all-gathered behind every score chunk) makes every rank's fr_worker_sync return FR_ERR_COMM.  The failure is injected in the
    EXPERIMENTS build (FR_SHARDED_INJECT_FC_FAIL=1; the product library has no such switch), in a child process, on a one-rank
    communicator: the failing rank is then its own peer -- submit returns the FC error, sync reports the status word, scores are NaN,
    and the communicator stays usable (nothing was aborted)."""
    import subprocess
    import sys
    exp = os.path.join(os.path.dirname(fr.LIB_PATH), "libfleetrec_exp.so")
    if not os.path.exists(exp):
        pytest.skip("experiments library not built (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
    code = r"""
import os, sys
import numpy as np
sys.path.insert(0, %r)
import __graft_entry__ as g
fr = g.load_package()
m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=30000)
ctx = fr.Context(m, device=%d, shard_rank=0, n_shards=1)
ctx.fill_tables(fr.FILL_HASH, 1); ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
comm = fr.Comm.init_rank(ctx, fr.Comm.unique_id())
rng = np.random.default_rng(3)
B = 200
idx = (rng.random((B, m.n_tables)) * m.rows()[None, :]).astype(np.int32)
dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
wk = fr.Worker(ctx, 256)
good = wk.infer_sharded(comm, idx, dense)
assert np.isfinite(good).all()
os.environ["FR_SHARDED_INJECT_FC_FAIL"] = "1"
wk.idx[:B] = idx; wk.dense[:B] = dense
rc = fr.lib().fr_worker_submit_sharded(wk._h, comm._h, B)
assert rc == fr.FR_ERR_STATE, rc
assert b"injected FC failure" in fr.lib().fr_last_error()
try:
    wk.sync()
    raise SystemExit("sync did not report the failed rank")
except fr.FleetRecError as ex:
    assert ex.status == fr.FR_ERR_COMM and "shard rank 0 reported a failed FC chain" in str(ex), ex
assert np.isnan(wk.score[:B]).all()
os.environ["FR_SHARDED_INJECT_FC_FAIL"] = "0"
again = wk.infer_sharded(comm, idx, dense)       # nothing was aborted: the communicator still works
assert np.array_equal(again, good)
# an argument error is returned as it is and leaves the communicator usable too
rc = fr.lib().fr_worker_submit_sharded(wk._h, comm._h, 100000)
assert rc == fr.FR_ERR_INVALID, rc
assert np.array_equal(wk.infer_sharded(comm, idx, dense), good)
print("ok")
""" % (ROOT, gpu)
    env = dict(os.environ, FR_LIB=exp)
    p = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_submit_sharded_through_rccl_two_ranks(fr, O, gpu, prec):
    """The G > 1 path of fr_comm_* + fr_worker_submit_sharded, which the one-GPU test boxes cannot run: two table-ID shards
    on two devices, fr_comm_init_all, one thread per rank, an UNEVEN split (B = 301: ranks take 151 and 150 items), the score all-gather.
    Skipped where fewer than two GPUs are visible -- the G > 1 RCCL path stays unmeasured on such boxes and DESIGN.md says so.
    Second half: a rank that does not take part (an argument error on that rank only: nothing is enqueued, its communicator stays usable)
    leaves its peer in the collective -- the peer's wait is BOUNDED (fr_comm_set_wait_ms) and ends in FR_ERR_COMM instead of hanging."""
    import threading
    if fr.device_count() < 2:
        pytest.skip("needs two GPUs: the G > 1 RCCL path is unmeasured on one-GPU boxes")
    G = 2
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=30000)
    om = O.OracleModel("C")
    P = {"f32": fr.FC_FP32, "bf16": fr.FC_BF16}[prec]
    ctxs_ = []
    for r in range(G):
        c = fr.Context(m, device=r, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        c.set_fc_precision(P)
        ctxs_.append(c)
    comms = fr.Comm.init_all(ctxs_)
    rng = np.random.default_rng(32)
    B = 301
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    wks = [fr.Worker(ctxs_[r], 512) for r in range(G)]
    got, errs = [None] * G, [None] * G

    def run(r, b):
        try:
            got[r] = wks[r].infer_sharded(comms[r], idx[:b], dense[:b])
        except Exception as ex:   # noqa: BLE001
            errs[r] = ex

    th = [threading.Thread(target=run, args=(r, B)) for r in range(G)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert errs == [None, None], errs
    assert np.array_equal(got[0], got[1])             # every rank ends with all B scores
    rec = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES).view(np.float32)
    ref = om.fc_chain(rec, [ctxs_[0].get_weights(l) for l in range(4)], acc64=True)
    assert rel_err(got[0], ref) <= {"f32": 1e-3, "bf16": 3e-2}[prec]
    # failure on one rank: rank 1 is handed a batch larger than its worker allows -> FR_ERR_INVALID there, nothing enqueued; rank 0's
    # collective never completes -> its bounded wait (3 s here) aborts its communicator and returns FR_ERR_COMM
    comms[0].set_wait_ms(3000)
    errs = [None] * G
    small = fr.Worker(ctxs_[1], 16)
    wks_bad = [wks[0], small]

    def run_bad(r):
        try:
            wks_bad[r].idx[:] = 0
            fr._check(fr.lib().fr_worker_submit_sharded(wks_bad[r]._h, comms[r]._h, 300))
            wks_bad[r].sync()
        except Exception as ex:   # noqa: BLE001
            errs[r] = ex

    th = [threading.Thread(target=run_bad, args=(r,)) for r in range(G)]
    [t.start() for t in th]
    [t.join(120) for t in th]
    assert not any(t.is_alive() for t in th), "a rank hung in the collective"
    assert errs[1] is not None and errs[1].status == fr.FR_ERR_INVALID
    assert errs[0] is not None and errs[0].status in (fr.FR_ERR_COMM, fr.FR_ERR_HIP), errs[0]
    for w_ in wks + [small]:
        w_.close()
    for c_ in comms:
        c_.close()
    for c_ in ctxs_:
        c_.close()


@pytest.mark.parametrize("G,prec", [(2, "f32"), (3, "bf16"), (8, "fp8"), (8, "f32")])
def test_submit_sharded_with_several_ranks_on_one_gpu_through_the_staged_exchange(fr, O, gpu, G, prec):
    """Round 6: fr_comm_init_all over GPU shard contexts that SHARE a device builds the staged host exchange (D2H -> rendezvous -> H2D; RCCL
    wants one device per rank), so the WHOLE step of fr_worker_submit_sharded runs with G = 2, 3, 8 ranks on the one GPU a test box has: slice
    gathers in the chain's operand type (fp32 / bf16 / e4m3 transport), the uneven item split (B = 301) and batches smaller than G on the
    device, the status words through the strided copy, the bf16 / fp8 chains on all-gathered slices, the sharded fp8 calibration (a
    synchronous collective: one thread per rank), submit on all ranks from ONE thread followed by the syncs (the step is issued by each
    worker's host stream).  Every rank ends with the same B scores; against the oracle within the chain's tolerance, in fp32 within 1e-5 of an
    unsharded context.  Then the failure protocol on the device: an injected FC failure on rank q -> every rank's sync names q, q's items are
    NaN (the device-side poisoning), the others right; a rank that never arrives trips the bounded wait."""
    import threading
    import time
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=20000)
    om = O.OracleModel("C")
    P = {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[prec]
    tol = {"f32": 1e-3, "bf16": 3e-2, "fp8": 0.15}[prec]
    ctxs_, wks = [], []
    for r in range(G):
        c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
        c.set_fc_precision(P)
        ctxs_.append(c)
        wks.append(fr.Worker(c, 1024))
    comms = fr.Comm.init_all(ctxs_)
    whole = fr.Context(m, device=gpu)
    whole.fill_tables(fr.FILL_HASH, SEED_TABLES)
    whole.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    w0 = fr.Worker(whole, 1024)
    rng = np.random.default_rng(60 + G)
    try:
        def load(idx, dense):
            for w in wks:
                w.idx[:len(idx)] = idx
                w.dense[:len(idx)] = dense
        if prec == "fp8":                                   # every rank calibrates on the same all-gathered fp32 slices: identical exponents
            idx_c = uniform_idx(rng, m.rows(), 1024)
            dense_c = rng.uniform(-1, 1, (1024, m.dense_len)).astype(np.float32)
            th = [threading.Thread(target=lambda r=r: wks[r].calibrate_fp8_sharded(comms[r], idx_c, dense_c)) for r in range(G)]
            [t.start() for t in th]
            [t.join(120) for t in th]
            assert not any(t.is_alive() for t in th)
            assert all(c.fp8_exponents() == ctxs_[0].fp8_exponents() for c in ctxs_)
        for B in (301, 5, 1024):
            idx = uniform_idx(rng, m.rows(), B)
            dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
            load(idx, dense)
            for r in range(G):                              # one driving thread: the submits return at once
                wks[r].submit_sharded(comms[r], B)
            got = []
            for r in reversed(range(G)):
                wks[r].sync()
                got.append(wks[r].score[:B].copy())
            for g_ in got[1:]:
                assert np.array_equal(g_, got[0]), (G, prec, B)
            rec = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES).view(np.float32)
            ref = om.fc_chain(rec, [ctxs_[0].get_weights(l) for l in range(4)], acc64=True)
            assert rel_err(got[0], ref) <= tol, (G, prec, B, rel_err(got[0], ref))
            if prec == "f32":
                assert rel_err(got[0], w0.infer(idx, dense)) <= 1e-5
        # kind (2): the FC chain of rank q "fails"
        B, q = 301, G - 1
        idx = uniform_idx(rng, m.rows(), B)
        dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
        load(idx, dense)
        for r in range(G):
            wks[r].submit_sharded(comms[r], B)
        for r in range(G):
            wks[r].sync()
        good = wks[0].score[:B].copy()
        wks[q].inject_fc_failure(1)
        for r in range(G):
            wks[r].submit_sharded(comms[r], B)
        base, rem = B // G, B % G
        lo = q * base + min(q, rem)
        hi = lo + base + (1 if q < rem else 0)
        for r in range(G):
            with pytest.raises(fr.FleetRecError) as e:
                wks[r].sync()
            assert e.value.status == fr.FR_ERR_COMM and "shard rank %d reported a failed FC chain" % q in str(e.value), (r, str(e.value))
            sc = wks[r].score[:B]
            assert np.isnan(sc[lo:hi]).all() and np.array_equal(sc[:lo], good[:lo]) and np.array_equal(sc[hi:], good[hi:]), r
        # kind (3): the last rank never arrives
        for cm in comms:
            cm.set_wait_ms(400)
        t0 = time.time()
        for r in range(G - 1):
            wks[r].submit_sharded(comms[r], B)
        for r in range(G - 1):
            with pytest.raises(fr.FleetRecError) as e:
                wks[r].sync()
            assert e.value.status == fr.FR_ERR_COMM, str(e.value)
        assert time.time() - t0 < 30
        with pytest.raises(fr.FleetRecError) as e:
            wks[G - 1].submit_sharded(comms[G - 1], B)
        assert e.value.status == fr.FR_ERR_COMM
    finally:
        for w in wks:
            w.close()
        for cm in comms:
            cm.close()
        for c in ctxs_:
            c.close()
        w0.close()
        whole.close()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_config4_shape_full_size_eight_ranks_through_the_c_abi_step(fr, O, gpu, ctxs, prec):
    """BASELINE configs[3] as the C-ABI runs it -- Model-C FULL SIZE (63.2 GB of tables cut into eight table-ID shards), batch 4096, eight ranks,
    fr_worker_submit_sharded on every rank -- on the one GPU of a test box through the staged exchange: every rank ends with the same 4096 scores;
    fp32 within 1e-5 of the unsharded full-size context, bf16 within 3e-2 of the fp64-accumulating oracle on EVERY item and within 1e-2 of the
    unsharded bf16 chain.  (What stays unmeasured is the transport -- RCCL over xGMI -- not the step.)"""
    G, B = 8, 4096
    m, whole = ctxs(2)
    om = O.OracleModel("C")
    P = {"f32": fr.FC_FP32, "bf16": fr.FC_BF16}[prec]
    ctxs_, wks = [], []
    comms = []
    rng = np.random.default_rng(4096)
    idx = uniform_idx(rng, m.rows(), B)
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    whole.set_fc_precision(P)
    try:
        w0 = fr.Worker(whole, B)
        unsharded = w0.infer(idx, dense)
        w0.close()
        for r in range(G):
            c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
            c.fill_tables(fr.FILL_HASH, SEED_TABLES)
            c.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
            c.set_fc_precision(P)
            ctxs_.append(c)
            wks.append(fr.Worker(c, B))
        comms = fr.Comm.init_all(ctxs_)
        for w in wks:
            w.idx[:B] = idx
            w.dense[:B] = dense
        for r in range(G):
            wks[r].submit_sharded(comms[r], B)
        got = []
        for r in range(G):
            wks[r].sync()
            got.append(wks[r].score[:B].copy())
        for g_ in got[1:]:
            assert np.array_equal(g_, got[0])
        rec = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES).view(np.float32)
        ref = om.fc_chain(rec, [whole.get_weights(l) for l in range(4)], acc64=True)
        assert rel_err(got[0], ref) <= {"f32": 1e-3, "bf16": 3e-2}[prec], rel_err(got[0], ref)
        assert rel_err(got[0], unsharded) <= {"f32": 1e-5, "bf16": 1e-2}[prec], rel_err(got[0], unsharded)
        if prec == "f32":
            assert rel_err_each(got[0], ref) <= 1e-3
    finally:
        whole.set_fc_precision(fr.FC_FP32)
        for w in wks:
            w.close()
        for cm in comms:
            cm.close()
        for c in ctxs_:
            c.close()


@pytest.mark.parametrize("rank", [1, 6])
def test_config5_inflated_shard_gather(fr, O, gpu, rank):
    """BASELINE configs[4] on one GPU: one of the 8 table-ID shards of Model-C inflated 5x (316 GB in total, 30-60 GB per shard).
    Indices run up to 500 M rows and row addresses far beyond 4 GiB inside the shard's arena; the slice must be bit-exact."""
    G = 8
    m = fr.Model.builtin(fr.MODEL_C).clone(row_scale=5.0)
    assert m.table_bytes() > 288e9
    offs, lens, F = m.shard_plan(G)
    c = fr.Context(m, device=gpu, shard_rank=rank, n_shards=G)
    c.fill_tables(fr.FILL_HASH, SEED_TABLES)
    rng = np.random.default_rng(500 + rank)
    B = 512
    rows = m.rows()
    idx = uniform_idx(rng, rows, B)
    idx[0], idx[1] = 0, rows - 1                      # first and last row of every table
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    wk = fr.Worker(c, B)
    sl = wk.gather_records(idx, dense).reshape(B, F)
    full = O.OracleModel("C").gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES)
    assert np.array_equal(sl[:, :lens[rank]], full[:, offs[rank]:offs[rank] + lens[rank]])
    bad = idx.copy()
    seg_tables = [sg.src for sg in m.segments() if sg.kind == fr.SEG_TABLE and offs[rank] <= sg.rec_offset < offs[rank] + lens[rank]]
    bad[7, seg_tables[0]] = rows[seg_tables[0]]       # one past the end of a table this shard owns
    with pytest.raises(fr.FleetRecError) as e:
        wk.gather_records(bad, dense)
    assert e.value.status == fr.FR_ERR_INDEX_RANGE
    wk.close()
    c.close()


def test_config5_all_shards_fp8_chain(fr, O, gpu):
    """BASELINE configs[4] completely, on the one GPU a test box has: Model-C with every table 5 x its rows (316 GB: past one GPU's
    288 GB), 8-way table-ID shards, batch 4096, fp8 FC.  All EIGHT inflated shards (30-60 GB each) take their turn on the device:
    create, fill, gather the shard's slice, keep it on the host, destroy -- twice: once in fp32 (the calibration pass every rank of
    the real job makes through fr_worker_calibrate_fp8_sharded) and once in e4m3 TRANSPORT with the calibrated X exponent, which is
    what travels through the all-gather.  Then the all-gathered layout [G][B][F] goes through fr_worker_fc_from_slices_lp for EVERY
    rank's B/G items, exactly as rank r of the 8-GPU job would run it.
    Checks: every fp32 slice bit-exact vs the oracle; every e4m3 slice = the documented encoding of the fp32 slice; fp8 scores from
    e4m3 transport == fp8 scores from fp32 slices bit for bit; vs the fp64-accumulating oracle <= 0.15 (fp8) and <= 3e-2 (the bf16
    chain on the same slices); fp8 vs bf16 chain <= 0.15."""
    import importlib
    dist_mod = importlib.import_module("fleetrec_amd.dist")
    G, B = 8, 4096
    m = fr.Model.builtin(fr.MODEL_C).clone(row_scale=5.0)
    assert m.table_bytes() > 288e9 and m.min_shards() > 1
    om = O.OracleModel("C")
    offs, lens, F = m.shard_plan(G)
    rng = np.random.default_rng(5005)
    rows = m.rows()
    idx = uniform_idx(rng, rows, B)
    idx[0], idx[1] = 0, rows - 1                      # first and last row of every (inflated) table
    dense = rng.uniform(-1, 1, (B, m.dense_len)).astype(np.float32)
    full = om.gather(idx, dense=dense, content_mode=O.FILL_HASH, seed=SEED_TABLES)

    def shard_pass(r, fn):
        c = fr.Context(m, device=gpu, shard_rank=r, n_shards=G)
        c.fill_tables(fr.FILL_HASH, SEED_TABLES)
        wk = fr.Worker(c, B)
        try:
            return fn(c, wk)
        finally:
            wk.close()
            c.close()

    # pass 1: fp32 slices (bit-exact vs the oracle) -> the calibration input
    slices = []
    for r in range(G):
        sl = shard_pass(r, lambda c, wk: wk.gather_records(idx, dense).reshape(B, F))
        assert np.array_equal(sl[:, :lens[r]], full[:, offs[r]:offs[r] + lens[r]]), r
        slices.append(sl)
    gathered32 = np.stack(slices)                     # [G][B][F] uint32 = what the fp32 all-gather delivers
    # the FC side: any shard's context serves (FC weights are replicated; its tables are never read by fc_from_slices) -- shard 0, unfilled
    cf = fr.Context(m, device=gpu, shard_rank=0, n_shards=G)
    cf.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    ws = [cf.get_weights(l) for l in range(4)]
    ref = om.fc_chain(full.view(np.float32), ws, acc64=True)
    wf = fr.Worker(cf, B)
    d_g32 = fr.DeviceBuffer.from_numpy(cf, gathered32)
    cf.set_fc_precision(fr.FC_FP8)
    wf.calibrate_fp8_slices(B, 0, B, d_g32)
    act_exp, w_exp = cf.fp8_exponents()

    def fc_all_ranks(d_gathered, transport):
        out = np.empty(B, np.float32)
        for r in range(G):                            # rank r's share of the batch, from the all-gathered layout
            lo, hi = dist_mod.item_range(r, G, B)
            d_s = fr.DeviceBuffer(cf, (hi - lo) * 4)
            wf.fc_from_slices_lp(B, lo, hi - lo, d_gathered, transport, d_s)
            wf.sync()
            out[lo:hi] = d_s.download(np.float32, hi - lo)
            d_s.free()
        return out

    fp8_from_f32 = fc_all_ranks(d_g32, fr.FC_FP32)
    # pass 2: every shard again, now emitting e4m3 slices with the calibrated X exponent (a quarter of the all-gather bytes)
    lp_slices = []
    for r in range(G):
        def emit(c, wk):
            c.set_fc_precision(fr.FC_FP8)
            c.set_fp8_act_exponents(act_exp)
            d_i = fr.DeviceBuffer.from_numpy(c, idx)
            d_d = fr.DeviceBuffer.from_numpy(c, dense)
            d_sl = fr.DeviceBuffer(c, B * F)
            wk.gather_slices(B, d_i, d_d, d_sl, fr.FC_FP8)
            wk.sync()
            return d_sl.download(np.uint8, B * F).reshape(B, F)
        s8 = shard_pass(r, emit)
        want8 = e4m3_encode(np.clip(slices[r][:, :lens[r]].view(np.float32).astype(np.float64) * 2.0 ** act_exp[0], -448, 448))
        assert np.array_equal(s8[:, :lens[r]], want8), r
        lp_slices.append(s8)
    d_g8 = fr.DeviceBuffer.from_numpy(cf, np.stack(lp_slices))
    fp8_scores = fc_all_ranks(d_g8, fr.FC_FP8)
    assert np.array_equal(fp8_scores, fp8_from_f32)   # the transport changes the bytes on the wire, not a bit of a score
    assert rel_err(fp8_scores, ref) <= 0.15, rel_err(fp8_scores, ref)
    # the bf16 chain on the same slices (bf16 wire format = RNE of the fp32 slice: test_table_sharded_mode_single_device_emulation pins that)
    cf.set_fc_precision(fr.FC_BF16)
    g16 = (bf16_round(gathered32.view(np.float32)).view(np.uint32) >> 16).astype(np.uint16)
    d_g16 = fr.DeviceBuffer.from_numpy(cf, g16)
    bf16_scores = fc_all_ranks(d_g16, fr.FC_BF16)
    assert rel_err(bf16_scores, ref) <= 3e-2, rel_err(bf16_scores, ref)
    assert rel_err(fp8_scores, bf16_scores) <= 0.15
    for b_ in (d_g32, d_g8, d_g16):
        b_.free()
    wf.close()
    cf.close()

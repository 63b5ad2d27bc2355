"""Multi-hot pooled lookups on the MI355X: gather_pooled_kernel (csrc/fr_gather.hip) behind fr_worker_gather_pooled /
fr_worker_submit_pooled_device / fr_worker_submit_pooled.  The same checks as tests/test_cpu_pooled.py (tests/pooled_helpers.py states the
contract in numpy), plus: the GPU's records against the CPU back-end's bit for bit, and the bf16 / fp8 chains from pooled records.

Bars: records bit-exact (uint32 equality); submit_pooled_device == fc_only on the records of gather_pooled == the host form, bit for bit,
in every precision; fp32 scores within BASELINE's 1e-3 of OracleModel.fc_chain (float64 accumulation) on the expected pooled records, in
the max-norm form (rel_err) as tests/test_gpu_scores.py applies it to one-hot scores, and item by item (rel_err_each) on the inputs of seed
29, for which tests/test_cpu_pooled.py::test_item_by_item_tolerance_precondition keeps the oracle's own fp32 chain inside 1e-3 of its
float64 chain."""
import numpy as np
import pytest
from conftest import free_port_block
from gpu_helpers import rel_err_each

import pooled_helpers as P

pytestmark = pytest.mark.gpu

CPU = -1
MODES = {"table": 0, "item": 1, "bank": 2}   # fr.INDEX_PER_TABLE / PER_ITEM / PER_BANK
ALL_FILLS = (0, 1, 2)                         # fr.FILL_EVEN_ODD / FILL_HASH / FILL_TAGGED


@pytest.mark.parametrize("mode", ["table", "bank", "item"])
@pytest.mark.parametrize("kind", [0, 1, 2, "spec"])
def test_one_hot_identity(fr, gpu, kind, mode):
    """Check 1.  Batch 1100 with Model-C's 992-word record takes the XCD-grouped grid, the narrow models the one-group grid."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], max_rows=30000)
    ctx = fr.Context(m, device=gpu)
    try:
        P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(3), 1100 if kind == 2 else 203, ALL_FILLS)
    finally:
        ctx.close()


def test_one_hot_identity_blocked_and_full_size(fr, gpu, ctxs):
    m = P.make_model(fr, 2, layout=fr.LAYOUT_BLOCKED, max_rows=30000)
    ctx = fr.Context(m, device=gpu)
    try:
        P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(4), 1100, ALL_FILLS)
    finally:
        ctx.close()
    m, ctx = ctxs(fr.MODEL_A)    # full size, hashed with SEED_TABLES (the identity check refills it with the same contents)
    P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(5), 2048, (fr.FILL_HASH,))


@pytest.mark.parametrize("kind,mode,blocked", [(0, "table", False), (1, "table", False), (1, "bank", False), (2, "table", False), (2, "bank", False),
                                                (2, "table", True), (0, "item", False), ("spec", "table", False), ("spec", "bank", False),
                                                ("spec", "item", False)])
def test_even_odd_known_answer(fr, gpu, kind, mode, blocked):
    """Check 2, mixed bags (spread_hots, 1 .. 64: the 16-slot window looped, 4-byte index loads) and uniform bags of 2 (the 2-slot window),
    of 4 and of 16 (16-byte index loads).  The 8-slot window and every other form: tests/test_gpu_gather_matrix.py::test_pooled_case."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], layout=fr.LAYOUT_BLOCKED if blocked else None, max_rows=30000)
    ctx = fr.Context(m, device=gpu)
    try:
        rng = np.random.default_rng(17)
        P.check_even_odd_known_answer(fr, ctx, m, rng, 1030 if kind == 2 else 90, P.spread_hots(m.idx_cols), blocked)
        for h in (2, 4, 16):
            P.check_even_odd_known_answer(fr, ctx, m, rng, 33, np.full(m.idx_cols, h, np.int32), blocked)
    finally:
        ctx.close()


def _scores_from_pooled(fr, O, ctx, m, which, hots, idx, dense, want, blocked, each):
    """Check 5 in the context's current precision; the oracle comparison (fp32 only) when `want` is given."""
    B = idx.shape[0]
    wk = fr.Worker(ctx, B)
    try:
        rec = wk.gather_pooled_records(idx, dense)
        d_i = fr.DeviceBuffer.from_numpy(ctx, idx)
        d_d = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        d_s = fr.DeviceBuffer(ctx, B * 4)
        wk.submit_pooled_device(B, d_i, d_d, d_s)
        wk.sync()
        dev = d_s.download(np.float32, B)
        assert np.isfinite(dev).all()
        assert np.array_equal(dev, wk.fc_scores(rec.view(np.float32)))
        assert np.array_equal(wk.infer_pooled(idx, dense), dev)
        if want is not None:
            x = (P.block_records(m, want) if blocked else want.ravel()).view(np.float32).reshape(B, m.record_len)
            ref = O.OracleModel(P.NAMES[which]).fc_chain(x, [ctx.get_weights(l) for l in range(4)], acc64=True)
            print("pooled fp32 scores vs oracle: max-norm %.3g" % P.rel_err(dev, ref))
            assert P.rel_err(dev, ref) <= 1e-3, P.rel_err(dev, ref)
            if each:
                print("pooled fp32 scores vs oracle: item by item %.3g" % rel_err_each(dev, ref))
                assert rel_err_each(dev, ref) <= 1e-3, rel_err_each(dev, ref)
        return dev
    finally:
        wk.close()


@pytest.mark.parametrize("which,mode,blocked", [(0, "table", False), (1, "table", False), (2, "table", False), (0, "bank", False), (1, "bank", False),
                                                 (2, "bank", False), (2, "table", True)])
def test_against_the_oracle_and_scores(fr, O, gpu, which, mode, blocked):
    """Checks 3 and 5 (fp32), the inputs of tests/test_cpu_pooled.py (seed 29 + model: item-by-item tolerance asserted for Model-A per-table,
    the case whose precondition the CPU module keeps)."""
    m = P.make_model(fr, which, index_mode=MODES[mode], layout=fr.LAYOUT_BLOCKED if blocked else None, max_rows=20000)
    ctx = fr.Context(m, device=gpu)
    try:
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        hots, idx, dense, want = P.check_against_oracle(fr, O, ctx, m, which, np.random.default_rng(29 + which), 48, per_bank=mode == "bank", blocked=blocked)
        ctx.set_pooling(hots)
        _scores_from_pooled(fr, O, ctx, m, which, hots, idx, dense, want, blocked, each=(which == 0 and mode == "table"))
    finally:
        ctx.close()


def test_against_the_oracle_full_size_model_a(fr, O, gpu, ctxs):
    """Check 3 on full-size Model-A (the session's shared context: pooling is cleared again before the test returns)."""
    m, ctx = ctxs(fr.MODEL_A)
    P.check_against_oracle(fr, O, ctx, m, 0, np.random.default_rng(31), 300, filled=True)
    assert ctx.pooled_index_cols == 0


@pytest.mark.parametrize("kind,mode,blocked", [(0, "table", False), (1, "bank", False), (2, "table", False), (2, "bank", False), (2, "table", True),
                                                ("spec", "table", False), ("spec", "bank", False), ("spec", "item", False)])
def test_gpu_equals_cpu_back_end(fr, gpu, kind, mode, blocked):
    """Check 4: the same inputs through gather_pooled_kernel and through frc_gather_pooled: the same bits (hashed tables)."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], layout=fr.LAYOUT_BLOCKED if blocked else None, max_rows=20000)
    rng = np.random.default_rng(53)
    B = 1040 if kind == 2 else 150
    out = []
    for hots in (P.spread_hots(m.idx_cols), np.full(m.idx_cols, 8, np.int32)):
        idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.2, empty_bags=10)
        dense = P.dense_for(rng, m, B)
        recs = []
        for dev in (gpu, CPU):
            ctx = fr.Context(m, device=dev)
            try:
                ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
                ctx.set_pooling(hots)
                wk = fr.Worker(ctx, B)
                recs.append(wk.gather_pooled_records(idx, dense))
                if dev == gpu:
                    assert wk.last_kernel().startswith("gather_pooled_kernel<"), wk.last_kernel()
                wk.close()
            finally:
                ctx.close()
        assert np.array_equal(recs[0], recs[1]), int((recs[0] != recs[1]).sum())
        out.append(recs[0])
    assert not np.array_equal(out[0][:1000], out[1][:1000])


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("which,B", [(0, 200), (2, 1024), (2, 100)])
def test_scores_in_every_precision(fr, O, gpu, which, B, prec):
    """Check 5: submit_pooled_device == fc_only on the records of gather_pooled, bit for bit, and the host form == the device form, in
    fp32, bf16 and fp8 (the chain model with its chain width set explicitly first)."""
    m = P.make_model(fr, which, max_rows=20000)
    ctx = fr.Context(m, device=gpu)
    try:
        ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        if which == 2:
            ctx.set_chain_width(1)
        ctx.set_fc_precision({"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[prec])
        rng = np.random.default_rng(61)
        if prec == "fp8":
            cal = fr.Worker(ctx, B)
            cal.calibrate_fp8((rng.random((B, m.idx_cols)) * m.index_ranges()[None, :]).astype(np.int32), P.dense_for(rng, m, B))
            cal.close()
        hots = np.array([1 + c % 4 for c in range(m.idx_cols)], np.int32)
        ctx.set_pooling(hots)
        idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.15, empty_bags=5)
        dense = P.dense_for(rng, m, B)
        _scores_from_pooled(fr, O, ctx, m, which, hots, idx, dense, None, False, False)
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_errors(fr, gpu, kind, mode):
    """Check 6."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], max_rows=2000)
    ctx = fr.Context(m, device=gpu)
    try:
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        P.check_errors(fr, ctx, m, np.random.default_rng(41))
    finally:
        ctx.close()


def test_sharded_contexts_refuse_pooling(fr, gpu):
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=500)
    ctx = fr.Context(m, device=gpu, shard_rank=1, n_shards=3)
    try:
        with pytest.raises(fr.FleetRecError) as e:
            ctx.set_pooling(np.ones(m.idx_cols, np.int32))
        assert e.value.status == fr.FR_ERR_STATE
    finally:
        ctx.close()


@pytest.mark.parametrize("ragged", [False, True])
def test_server_answers_pooled_requests_on_the_gpu(fr, gpu, ragged):
    """Check 7 on the GPU: fleetrec_server --device 0 --hots 4 fed by fleetrec_sender --hots 4 [--ragged] over loopback."""
    P.check_server(fr, gpu, ragged, free_port_block)

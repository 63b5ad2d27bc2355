"""Multi-hot pooled lookups (fr_ctx_set_pooling / fr_worker_gather_pooled / fr_worker_submit_pooled*, include/fleetrec_serving.h) on the
CPU back-end (device = -1, csrc/fr_cpu.cpp frc_gather_pooled).  Runs without a GPU; tests/test_gpu_pooled.py runs the same checks
(tests/pooled_helpers.py) on the MI355X and compares the two back-ends bit for bit.

Bars: records bit-exact (uint32 equality) against the one-hot gather (hots = 1), against the even/odd known answer and against
OracleModel.gather run once per slot and folded in numpy by the contract's rule (copy the first non-empty slot, then one fp32 add per
further slot, in slot order); fp32 scores against OracleModel.fc_chain (float64 accumulation) on the expected pooled records within
BASELINE's 1e-3, in its max-norm form (rel_err), as tests/test_gpu_scores.py applies it to one-hot scores."""
import numpy as np
import pytest
from conftest import free_port_block

import pooled_helpers as P

CPU = -1
MODES = {"table": 0, "item": 1, "bank": 2}   # fr.INDEX_PER_TABLE / PER_ITEM / PER_BANK


@pytest.mark.parametrize("mode", ["table", "bank", "item"])
@pytest.mark.parametrize("kind", [0, 1, 2, "spec"])
def test_one_hot_identity(fr, kind, mode):
    """Check 1: shrunk Models A / B / C and the mixed-width user model, PER_TABLE / PER_BANK / PER_ITEM, EVEN_ODD / HASH / TAGGED."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], max_rows=3000)
    ctx = fr.Context(m, device=CPU)
    try:
        P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(3), 70, (fr.FILL_EVEN_ODD, fr.FILL_HASH, fr.FILL_TAGGED))
    finally:
        ctx.close()


def test_one_hot_identity_blocked_and_full_size(fr):
    """Check 1 on Model-C's BLOCKED layout (the 3-node receive buffer) and on full-size Model-A (1.4 GB of tables, hashed)."""
    m = P.make_model(fr, 2, layout=fr.LAYOUT_BLOCKED, max_rows=3000)
    ctx = fr.Context(m, device=CPU)
    try:
        P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(4), 70, (fr.FILL_EVEN_ODD, fr.FILL_HASH, fr.FILL_TAGGED))
    finally:
        ctx.close()
    m = fr.Model.builtin(fr.MODEL_A)
    ctx = fr.Context(m, device=CPU)
    try:
        P.check_one_hot_identity(fr, ctx, m, np.random.default_rng(5), 130, (fr.FILL_HASH,))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,mode,blocked", [(0, "table", False), (1, "table", False), (1, "bank", False), (2, "table", False), (2, "bank", False),
                                                (2, "table", True), (0, "item", False), ("spec", "table", False), ("spec", "bank", False),
                                                ("spec", "item", False)])
def test_even_odd_known_answer(fr, kind, mode, blocked):
    """Check 2: every pooled table word counts the even indices among its bag's non-empty slots; Model-B's pad word follows PLRAM16's
    bag (a COPY word takes its source table's column); Model-C's dense words are the request's."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], layout=fr.LAYOUT_BLOCKED if blocked else None, max_rows=3000)
    ctx = fr.Context(m, device=CPU)
    try:
        rng = np.random.default_rng(17)
        P.check_even_odd_known_answer(fr, ctx, m, rng, 90, P.spread_hots(m.idx_cols), blocked)
        P.check_even_odd_known_answer(fr, ctx, m, rng, 33, np.full(m.idx_cols, 4, np.int32), blocked)   # uniform bags: the 16-byte index loads' shape
    finally:
        ctx.close()


@pytest.mark.parametrize("which,mode,blocked", [(0, "table", False), (1, "table", False), (2, "table", False), (0, "bank", False), (1, "bank", False),
                                                 (2, "bank", False), (2, "table", True)])
def test_against_the_oracle_and_scores(fr, O, which, mode, blocked):
    """Checks 3 and 5 (fp32): hashed tables, hots 1 / 2 / 3 / 8 / 64 spread over the columns, ragged bags, some entirely empty.  Records
    bit-exact against the per-slot oracle gathers folded in numpy; submit_pooled_device == fc_only on those records == submit_pooled
    (host form), bit for bit; scores within 1e-3 (max-norm) of the oracle's float64-accumulating chain on the expected records."""
    per_bank = mode == "bank"
    m = P.make_model(fr, which, index_mode=MODES[mode], layout=fr.LAYOUT_BLOCKED if blocked else None, max_rows=20000)
    ctx = fr.Context(m, device=CPU)
    try:
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        rng = np.random.default_rng(29 + which)
        B = 48
        hots, idx, dense, want = P.check_against_oracle(fr, O, ctx, m, which, rng, B, per_bank=per_bank, blocked=blocked)
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, B)
        rec = wk.gather_pooled_records(idx, dense)
        d_i = fr.DeviceBuffer.from_numpy(ctx, idx)
        d_d = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        d_s = fr.DeviceBuffer(ctx, B * 4)
        wk.submit_pooled_device(B, d_i, d_d, d_s)
        wk.sync()
        dev = d_s.download(np.float32, B)
        assert np.array_equal(dev, wk.fc_scores(rec.view(np.float32)))
        assert np.array_equal(wk.infer_pooled(idx, dense), dev)
        x = (P.block_records(m, want) if blocked else want.ravel()).view(np.float32).reshape(B, m.record_len)   # what the chain reads as B x K
        ref = O.OracleModel(P.NAMES[which]).fc_chain(x, [ctx.get_weights(l) for l in range(4)], acc64=True)
        print("pooled scores vs oracle (max-norm):", P.rel_err(dev, ref))
        assert P.rel_err(dev, ref) <= 1e-3, P.rel_err(dev, ref)
        wk.close()
    finally:
        ctx.close()


def test_item_by_item_tolerance_precondition(fr, O):
    """Check 5's item-by-item form (gpu_helpers.rel_err_each) divides by each item's own score, and sums of zero-mean hashed rows can land
    near zero, so tests/test_gpu_pooled.py asserts it only on inputs for which the ORACLE's fp32 chain already stays inside 1e-3 of its
    own float64 chain.  That was checked here for seed 29 (Model-A, per-table, the inputs of test_against_the_oracle_and_scores): this test
    keeps the precondition true, and the CPU back-end's scores inside the same bound."""
    from gpu_helpers import rel_err_each
    m = P.make_model(fr, 0, max_rows=20000)
    ctx = fr.Context(m, device=CPU)
    try:
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        hots, idx, dense, want = P.check_against_oracle(fr, O, ctx, m, 0, np.random.default_rng(29), 48)
        om = O.OracleModel("A")
        ws = [ctx.get_weights(l) for l in range(4)]
        x = want.view(np.float32)
        ref = om.fc_chain(x, ws, acc64=True)
        pre = rel_err_each(om.fc_chain(x, ws, acc64=False), ref)
        print("oracle fp32 chain vs its float64 chain, item by item:", pre)
        assert pre <= 1e-3, pre
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, 48)
        got = wk.infer_pooled(idx, dense)
        print("CPU back-end, item by item:", rel_err_each(got, ref))
        assert rel_err_each(got, ref) <= 1e-3
        wk.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_errors(fr, kind, mode):
    """Check 6."""
    m = P.make_model(fr, kind, index_mode=MODES[mode], max_rows=2000)
    ctx = fr.Context(m, device=CPU)
    try:
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        P.check_errors(fr, ctx, m, np.random.default_rng(41))
    finally:
        ctx.close()


def test_sharded_contexts_refuse_pooling(fr):
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=500)
    ctx = fr.Context(m, device=CPU, shard_rank=1, n_shards=3)
    try:
        with pytest.raises(fr.FleetRecError) as e:
            ctx.set_pooling(np.ones(m.idx_cols, np.int32))
        assert e.value.status == fr.FR_ERR_STATE
        assert ctx.pooled_index_cols == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("ragged", [False, True])
def test_server_answers_pooled_requests_on_the_cpu_back_end(fr, ragged):
    """Check 7: fleetrec_server --device -1 --hots 4 fed by fleetrec_sender --hots 4 [--ragged] over loopback."""
    P.check_server(fr, CPU, ragged, free_port_block)


def test_server_refuses_hots_with_stream_or_shards(fr):
    P.check_server_refuses_stream(fr)

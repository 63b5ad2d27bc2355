"""Sparse row updates on the MI355X: the checks of tests/update_rows.py on the device (the scatter arm of fill_table_kernel in the plain and the
bank-interleaved layout), and what only the device has -- the operand-type bank image patched in place by the listed-rows arm of
convert_rows_lp_kernel<1|2> instead of rebuilt, and a rebuild ordered behind the updates in flight on other workers."""
import numpy as np
import pytest
from conftest import free_port_block

import gather_matrix as G
import update_rows as U

pytestmark = pytest.mark.gpu

LP_FORMS = [(1, 0), (2, -8), (2, 3)]      # (transport, X exponent): bf16; e4m3 at exponents -8 and 3
LP_IDS = ["bf16", "fp8-e-8", "fp8-e3"]
B_IMG = 8192                              # the batch at which test_operand_image_rounding_exhaustive shows the chain reading the image


@pytest.mark.parametrize("form", U.FORMS)
@pytest.mark.parametrize("mode", ["bank", "table"])
def test_addressing(fr, gpu, mode, form):
    U.check_addressing(fr, gpu, mode, form)


def test_range_and_arguments(fr, gpu):
    U.check_range_and_arguments(fr, gpu)


def test_duplicates(fr, gpu):
    U.check_duplicates(fr, gpu)


@pytest.mark.parametrize("group", [64, 1])
def test_order_on_one_worker(fr, gpu, group):
    U.check_order_on_one_worker(fr, gpu, group)


def test_server_update_port(fr, gpu):
    U.check_server(fr, gpu, free_port_block)


# ---- the operand-type bank image ---------------------------------------------------------------------------------------------------------

def _same_codes(got, bits, tp, e_x, what):
    """the comparison of tests/test_gpu_gather_matrix.py, restated: the device's codes against gather_matrix.lp_expected, NaN codes canonical"""
    want, nan = G.lp_expected(bits, tp, e_x)
    got = G.canon(got, nan, tp)
    assert np.array_equal(got, want), "%s: %d of %d codes differ" % (what, int((got != want).sum()), want.size)


def _lp_context(fr, gpu, m, tables, tp, e_x):
    ctx = fr.Context(m, device=gpu)
    for t, a in enumerate(tables):
        ctx.upload_table(t, a)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 1)
    ctx.set_fc_precision(fr.FC_BF16 if tp == 1 else fr.FC_FP8)
    if tp == 2:
        ctx.set_fp8_act_exponents([e_x, 0, 0, 0])
    return ctx


def _batch(m, n_rows):
    rows = (np.arange(B_IMG) % n_rows).astype(np.int32)
    return rows, np.repeat(rows[:, None], m.idx_cols, axis=1)


def _features(wk, m, tp):
    return wk.features(B_IMG, bf16=tp == 1, fp8=tp == 2)[:m.record_len].T


def _patch_rows(exh, t):
    """257 source rows of the exhaustive table, rolled by the table number: rows 0, 24, 48, ... of every region of the fp32 line, and the rows
    that hold the infinities and the NaN patterns of either sign -- every fp32 class passes through the patch"""
    src_rows = (np.arange(257) * 24) % exh.shape[0]
    src_rows[-8:] = [3060, 3064, 3068, 3071, 6132, 6136, 6140, 6143]
    return np.roll(exh, 1000 + t, axis=0)[src_rows]


@pytest.mark.parametrize("tp,e_x", LP_FORMS, ids=LP_IDS)
def test_bank_image_is_patched_not_rebuilt(fr, gpu, tp, e_x):
    """Check 5: with the image in place, 257 rows of two tables are updated (one through each form); the next batch finds the image current --
    the build count stands -- and its operand image holds the codes of the new contents; scores equal those of the image switched off and those
    of a fresh context given the final tables by upload; an upload of the same table DOES count a build; an update before the first image
    exists leaves one build with the same codes."""
    exh = G.exhaustive_bits()
    m = G.make_model(fr, "exh256", "bank")
    tables = [np.roll(exh, t, axis=0).copy() for t in range(m.n_tables)]
    rows, idx = _batch(m, exh.shape[0])
    rng = np.random.default_rng(4500 + tp + e_x)
    ctx = _lp_context(fr, gpu, m, tables, tp, e_x)
    ctx2 = ctx3 = None
    try:
        wk = fr.Worker(ctx, B_IMG)
        wk.infer(idx)
        assert ctx.lp_bank_image_bytes() > 0
        builds = ctx.lp_bank_image_builds()
        assert builds == 1
        updates = []
        for t, form in ((1, "worker"), (3, "host")):
            ids = rng.permutation(exh.shape[0])[:257].astype(np.int32)
            src = _patch_rows(exh, t)
            U.update(fr, ctx, wk, form, t, ids, src)
            tables[t][ids] = src
            updates.append((t, ids, src))
        s1 = wk.infer(idx).view(np.uint32)
        assert ctx.lp_bank_image_builds() == builds, "the update made the next launch rebuild the image"
        bits = np.concatenate([tables[t][rows] for t in range(m.n_tables)], axis=1)
        _same_codes(_features(wk, m, tp), bits, tp, e_x, "patched image")
        U.assert_tables(ctx, m, tables, "the fp32 arena")
        ctx.set_lp_bank_image(0)
        s_off = wk.infer(idx).view(np.uint32)
        ctx.set_lp_bank_image(1)
        assert np.array_equal(s1, s_off), "scores through the patched image differ from the fp32 rows'"
        # a fresh context given the final tables by upload
        ctx2 = _lp_context(fr, gpu, m, tables, tp, e_x)
        wk2 = fr.Worker(ctx2, B_IMG)
        assert np.array_equal(wk2.infer(idx).view(np.uint32), s1), "scores differ from a context that was uploaded the final tables"
        wk2.close()
        # the update before the first image exists: one build, the same codes
        ctx3 = _lp_context(fr, gpu, m, [np.roll(exh, t, axis=0) for t in range(m.n_tables)], tp, e_x)
        wk3 = fr.Worker(ctx3, B_IMG)
        for t, ids, src in updates:
            U.update(fr, ctx3, wk3, "worker", t, ids, src)
        assert ctx3.lp_bank_image_builds() == 0
        assert np.array_equal(wk3.infer(idx).view(np.uint32), s1)
        assert ctx3.lp_bank_image_builds() == 1
        _same_codes(_features(wk3, m, tp), bits, tp, e_x, "image built after the update")
        wk3.close()
        # control: the counter counts -- an upload of the same table makes the next launch rebuild
        ctx.upload_table(1, tables[1])
        assert np.array_equal(wk.infer(idx).view(np.uint32), s1)
        assert ctx.lp_bank_image_builds() == builds + 1
        wk.close()
    finally:
        for c in (ctx, ctx2, ctx3):
            if c is not None:
                c.close()


@pytest.mark.parametrize("tp,e_x", [(1, 0), (2, 0)], ids=["bf16", "fp8"])
def test_duplicates_in_the_bank_image(fr, gpu, tp, e_x):
    """Check 3 (image side): an id listed twice with two different source rows -- whichever words the fp32 arena ends up with, the operand image
    of the following batch holds their codes (the patch reads the arena, not the caller's rows)."""
    exh = G.exhaustive_bits()
    m = G.make_model(fr, "exh256", "bank")
    tables = [np.roll(exh, t, axis=0) for t in range(m.n_tables)]
    rows, idx = _batch(m, exh.shape[0])
    ctx = _lp_context(fr, gpu, m, tables, tp, e_x)
    try:
        wk = fr.Worker(ctx, B_IMG)
        wk.infer(idx)
        builds = ctx.lp_bank_image_builds()
        ids = np.array([5, 9, 5, 4000, 4000, 4000], np.int32)
        src = np.roll(exh, 77, axis=0)[[100, 2000, 3064, 4500, 6140, 30]]
        for form in U.FORMS:
            U.update(fr, ctx, wk, form, 2, ids, src)
            wk.infer(idx)
            assert ctx.lp_bank_image_builds() == builds
            got = U.download_all(ctx, m)
            for r, listed in ((5, (0, 2)), (4000, (3, 4, 5))):
                g = got[2][r].reshape(-1, 4)
                assert np.logical_or.reduce([(g == src[i].reshape(-1, 4)).all(axis=1) for i in listed]).all()
            assert np.array_equal(got[2][9], src[1])
            bits = np.concatenate([got[t][rows] for t in range(m.n_tables)], axis=1)
            _same_codes(_features(wk, m, tp), bits, tp, e_x, "%s form" % form)
            src = src[::-1].copy()
        wk.close()
    finally:
        ctx.close()


def test_tail_rows_leave_the_image_alone(fr, gpu):
    """Check 5, last item: ids at or past the bank's common range (the tail of a bank-interleaved table) are written to the fp32 arena and dropped
    by the image patch -- the image holds no such row: the operand image of the next batch is unchanged, nothing is rebuilt, nothing faults."""
    il, tail = 6144, 56
    spec = {"name": "ur_tail", "tables": [{"dim": 64, "rows": il, "bank": 0}, {"dim": 64, "rows": il + tail, "bank": 0},
                                          {"dim": 64, "rows": il, "bank": 1}, {"dim": 64, "rows": il, "bank": 2}], "fc": [2048, 512, 256]}
    m = fr.Model.from_spec(spec).clone(index_mode=fr.INDEX_PER_BANK)
    rng = np.random.default_rng(4600)
    tables = [(3.0 * rng.standard_normal((int(t.rows), t.dim))).astype(np.float32).view(np.uint32) for t in m.tables()]
    rows, idx = _batch(m, il)
    ctx = _lp_context(fr, gpu, m, tables, 1, 0)
    try:
        wk = fr.Worker(ctx, B_IMG)
        wk.infer(idx)
        assert ctx.lp_bank_image_bytes() > 0
        builds = ctx.lp_bank_image_builds()
        before = _features(wk, m, 1).copy()
        ids = np.arange(il, il + tail, dtype=np.int32)
        for form in U.FORMS:
            src = rng.integers(0, 2 ** 32, size=(tail, 64), dtype=np.uint32)
            U.update(fr, ctx, wk, form, 1, ids, src)
            tables[1][ids] = src
            U.assert_tables(ctx, m, tables, "%s form, tail rows" % form)
            wk.infer(idx)
            assert ctx.lp_bank_image_builds() == builds
            assert np.array_equal(_features(wk, m, 1), before)
        # a list that mixes the last image row with tail rows: the one is patched, the others are dropped
        ids = np.array([il - 1, il, il + tail - 1], np.int32)
        src = (3.0 * rng.standard_normal((3, 64))).astype(np.float32).view(np.uint32)
        U.update(fr, ctx, wk, "worker", 1, ids, src)
        tables[1][ids] = src
        wk.infer(idx)
        assert ctx.lp_bank_image_builds() == builds
        bits = np.concatenate([tables[t][rows] for t in range(m.n_tables)], axis=1)
        _same_codes(_features(wk, m, 1), bits, 1, 0, "the last image row beside tail rows")
        wk.close()
    finally:
        ctx.close()


def test_a_rebuild_waits_for_updates_in_flight(fr, gpu):
    """Check 6: worker A enqueues an update and does not sync; the X exponent changes, so the image is stale; worker B's next batch rebuilds it
    on the set-up stream -- behind A's update: B's operand image holds the NEW contents at the NEW exponent."""
    exh = G.exhaustive_bits()
    m = G.make_model(fr, "exh256", "bank")
    tables = [np.roll(exh, t, axis=0).copy() for t in range(m.n_tables)]
    rows, idx = _batch(m, exh.shape[0])
    ctx = _lp_context(fr, gpu, m, tables, 2, 0)
    try:
        wa, wb = fr.Worker(ctx, B_IMG), fr.Worker(ctx, B_IMG)
        wb.infer(idx)
        builds = ctx.lp_bank_image_builds()
        ids = np.arange(exh.shape[0], dtype=np.int32)[::-1].copy()          # every row of the table: a scatter worth waiting for
        src = np.roll(exh, 3000, axis=0)
        d_ids, d_src = fr.DeviceBuffer.from_numpy(ctx, ids), fr.DeviceBuffer.from_numpy(ctx, src)
        wa.update_rows(2, len(ids), d_ids, d_src)
        ctx.set_fp8_act_exponents([3, 0, 0, 0])
        wb.infer(idx)
        wa.sync()
        tables[2][ids] = src
        assert ctx.lp_bank_image_builds() == builds + 1
        bits = np.concatenate([tables[t][rows] for t in range(m.n_tables)], axis=1)
        _same_codes(_features(wb, m, 2), bits, 2, 3, "image rebuilt beside an update in flight")
        U.assert_tables(ctx, m, tables, "the fp32 arena")
        d_ids.free()
        d_src.free()
        wa.close()
        wb.close()
    finally:
        ctx.close()

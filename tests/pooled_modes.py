"""Shared by tests/test_cpu_pooled_modes.py and tests/test_gpu_pooled_modes.py: pooling modes (SUM / MEAN) and per-sample weights of the
multi-hot lookups, restated in numpy, and the checks written once for both back-ends (device = -1: the CPU back-end).

Contract (include/fleetrec_serving.h).  WEIGHTED: a non-empty slot's term is w * x, ONE np.float32 multiply per lane; the first non-empty
slot's term is the accumulator (not a bit copy), every further term is added with one np.float32 add, in ascending slot order; an empty
slot's weight is never read (the generator below puts a NaN there); an all-empty bag gives +0.0f; DENSE words are copied unweighted.
MEAN: the SUM fold (tests/pooled_helpers.py) divided by n, the bag's count of non-empty slots, one np.float32 division; n == 1 leaves the
bit copy, n == 0 gives +0.0f; DENSE words are never divided.  As in pooled_helpers.expected_from_onehot each slot level is applied to
the one-hot expectation of that level.  Bits are pinned wherever the expectation is not a NaN; where it is, the result must be a NaN."""
import ctypes
import functools

import numpy as np
import pytest

import gather_matrix as GM
import pooled_helpers as P

CPU = -1
SUM, MEAN = 0, 1


# ---- the contract in numpy -------------------------------------------------------------------------------------------------------------

def fold_weighted(slot_records, slot_valid, slot_weights):
    """slot_records / slot_valid as pooled_helpers.fold_slots; slot_weights: list of float32 [B][K], the weight every float's bag gives
    its slot of that level.  -> uint32 [B][K]."""
    acc = np.zeros_like(slot_records[0], dtype=np.uint32)
    have = np.zeros(acc.shape, dtype=bool)
    for v, ok, w in zip(slot_records, slot_valid, slot_weights):
        with np.errstate(all="ignore"):
            term = np.multiply(w, v.view(np.float32), dtype=np.float32)            # ONE fp32 multiply per lane, rounded on its own
            s = np.add(acc.view(np.float32), term, dtype=np.float32)               # ... then ONE fp32 add
        nxt = np.where(have, s.view(np.uint32), term.view(np.uint32))
        acc = np.where(ok, nxt, acc)
        have |= ok
    return acc


def _levels(fr, m, hots, idx, gather_onehot, weights=None):
    """-> per slot level: the one-hot records, the validity of that slot for every float, (the weight of that slot for every float)."""
    hots = np.asarray(hots, dtype=np.int64)
    pre = P.prefix_of(hots)
    col = P.column_of_float(fr, m)
    tab = col >= 0
    B = idx.shape[0]
    recs, oks, wts = [], [], []
    for j in range(int(hots.max())):
        one = np.zeros((B, len(hots)), dtype=np.int32)
        valid = np.zeros((B, len(hots)), dtype=bool)
        wj = np.ones((B, len(hots)), dtype=np.float32)
        for c, h in enumerate(hots):
            if j < h:
                s = idx[:, pre[c] + j]
                valid[:, c] = s != -1
                one[:, c] = np.where(s != -1, s, 0)
                if weights is not None:
                    wj[:, c] = weights[:, pre[c] + j]
        r = gather_onehot(one)
        ok = np.zeros(r.shape, dtype=bool)
        ok[:, tab] = valid[:, col[tab]]
        w = np.ones(r.shape, dtype=np.float32)
        w[:, tab] = wj[:, col[tab]]
        recs.append(r)
        oks.append(ok)
        wts.append(w)
    return recs, oks, wts, col


def _with_dense(out, col, dense):
    if (col < 0).any():
        out[:, col < 0] = np.ascontiguousarray(dense, dtype=np.float32).reshape(out.shape[0], -1).view(np.uint32)
    return out


def expected_weighted(fr, m, hots, idx, weights, dense, gather_onehot):
    """Expected weighted records, uint32 [B][K] in SEMANTIC order.  gather_onehot(int32 [B][cols]) -> uint32 [B][K]."""
    recs, oks, wts, col = _levels(fr, m, hots, idx, gather_onehot, np.ascontiguousarray(weights, np.float32))
    return _with_dense(fold_weighted(recs, oks, wts), col, dense)


def bag_counts(hots, idx):
    """int [B][cols]: the non-empty slots of every bag."""
    pre = P.prefix_of(hots)
    return np.stack([(idx[:, pre[c]:pre[c] + int(h)] != -1).sum(axis=1) for c, h in enumerate(hots)], axis=1)


def expected_modes(fr, m, hots, modes, idx, dense, gather_onehot, sum_records=None):
    """Expected unweighted records under per-column modes: the SUM fold, MEAN columns' table / copy floats divided by n where n >= 2."""
    if sum_records is None:
        sum_records = P.expected_from_onehot(fr, m, hots, idx, dense, gather_onehot)
    col = P.column_of_float(fr, m)
    tab = col >= 0
    n = np.zeros(sum_records.shape, dtype=np.int64)
    n[:, tab] = bag_counts(hots, idx)[:, col[tab]]
    is_mean = np.zeros(sum_records.shape, dtype=bool)
    is_mean[:, tab] = (np.asarray(modes)[col[tab]] == MEAN)[None, :]
    div = is_mean & (n >= 2)
    with np.errstate(all="ignore"):
        q = np.divide(sum_records.view(np.float32), np.maximum(n, 1).astype(np.float32), dtype=np.float32)   # ONE fp32 division, n exact
    return np.where(div, q.view(np.uint32), sum_records)


def is_nan_bits(u):
    u = np.asarray(u, np.uint32)
    return ((u & 0x7F800000) == 0x7F800000) & ((u & 0x007FFFFF) != 0)


def assert_bits(got, want, what=""):
    """Equal bits where the expectation is not a NaN, a NaN (any payload) where it is."""
    got, want = np.asarray(got, np.uint32).ravel(), np.asarray(want, np.uint32).ravel()
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = is_nan_bits(want)
    bad = (got != want) & ~nan
    assert not bad.any(), "%s: %d words differ, first at %d: got %08x want %08x" % (what, int(bad.sum()), int(np.flatnonzero(bad)[0]),
                                                                                  int(got[bad][0]), int(want[bad][0]))
    assert is_nan_bits(got[nan]).all(), "%s: a NaN expectation came back as a number" % what


def make_weights(rng, hots, idx, special=()):
    """float32 [B][P] for pooled rows idx: ordinary weights in +-[2^-4, 4], exact zeros, weights near 2^-125 (a product with an N(0, 3)
    row value is then a subnormal or rounds into one), and a NaN on EVERY empty slot.  A bag that holds one of the rows `special`
    (NaN, +-inf, -0.0, a subnormal) gets +1.0 or -1.0 on all its slots, so that the expectation stays defined (0 x inf is none)."""
    B, Pn = idx.shape
    w = (np.exp2(rng.uniform(-4.0, 2.0, (B, Pn))) * rng.choice([-1.0, 1.0], (B, Pn))).astype(np.float32)
    kind = rng.random((B, Pn))
    w[kind < 0.06] = 0.0
    w[(kind >= 0.06) & (kind < 0.08)] = -0.0
    tiny = (kind >= 0.08) & (kind < 0.14)
    w[tiny] = (np.exp2(rng.uniform(-127.0, -123.0, int(tiny.sum()))) * rng.choice([-1.0, 1.0], int(tiny.sum()))).astype(np.float32)
    if len(special):
        pre = P.prefix_of(hots)
        for c, h in enumerate(hots):
            bag = idx[:, pre[c]:pre[c] + int(h)]
            hit = np.isin(bag, list(special)).any(axis=1)
            sign = np.where((np.arange(B) + c) % 2 == 0, 1.0, -1.0).astype(np.float32)
            w[hit, pre[c]:pre[c] + int(h)] = sign[hit, None]
    w[idx == -1] = np.float32(np.nan)
    return w


# ---- checks 1 and 2: every POOLED_CASES entry, weighted / MEAN / alternating SUM and MEAN ------------------------------------------------

@functools.lru_cache(maxsize=3)
def _case_arrays(fr, case_id):
    case = next(c for c in GM.POOLED_CASES if c["id"] == case_id)
    m = GM.make_model(fr, case["model"], case["mode"])
    tables, hots, idx, dense = GM.pooled_data(m, case)
    rng = np.random.default_rng(GM.case_seed(case) + 77)
    weights = make_weights(rng, hots, idx, special=tuple(GM.SPECIAL_ROWS))
    want_sum = P.expected_from_onehot(fr, m, hots, idx, dense, lambda one: GM.expected_records(m, tables, one, dense))
    return case, tables, hots, idx, dense, weights, want_sum


def case_inputs(fr, case_id):
    """The case's own model, tables, hots, rows and dense features (gather_matrix.pooled_data), its weights, and the SUM expectation; the
    arrays are computed once and shared by the weighted and the mode tests of the case (nothing here is modified afterwards)."""
    case, tables, hots, idx, dense, weights, want_sum = _case_arrays(fr, case_id)
    m = GM.make_model(fr, case["model"], case["mode"])
    return case, m, tables, hots, idx, dense, weights, (lambda one: GM.expected_records(m, tables, one, dense)), want_sum


def _device_rows(fr, ctx, arr, shift=0):
    """arr on the device at an address `shift` bytes past a 16-byte boundary.  -> (allocation, address)."""
    flat = np.ascontiguousarray(arr)
    raw = fr.DeviceBuffer(ctx, flat.nbytes + 256)
    base = (raw.ptr.value + 15) // 16 * 16 + shift
    fr._check(fr.lib().fr_memcpy_h2d(ctx._h, ctypes.c_void_p(base), flat.ctypes.data_as(ctypes.c_void_p), flat.nbytes))
    return raw, base


def _check_guarded(dst, want, K):
    """Margins and bits through Guarded.check (the NaN expectations skipped there), then the NaN expectations: a NaN came back."""
    nan = is_nan_bits(want)
    dst.check(lambda b0, n: want[b0:b0 + n], K * 4, skip=np.repeat(nan, 4, axis=1) if nan.any() else None)
    if nan.any():
        got = dst.buf.download(np.uint8, dst.total)[dst.pre:dst.pre + dst.B * dst.stride].view(np.uint32).reshape(dst.B, -1)[:, :K]
        assert is_nan_bits(got[nan]).all(), "a NaN expectation came back as a number"


def run_case_weighted(fr, device, case_id):
    """Check 1: the case's batches through the weighted gather into a guarded destination; on the GPU the kernel is the case's own; for
    the 16-byte forms once more with the weights 4 bytes past a 16-byte boundary (index rows aligned): the narrow kernel, the same bits."""
    case, m, tables, hots, idx, dense, weights, onehot, _ = case_inputs(fr, case_id)
    want = expected_weighted(fr, m, hots, idx, weights, dense, onehot)
    assert np.isnan(weights[idx == -1]).all() and (idx == -1).any()
    K = m.record_len
    ctx = fr.Context(m, device=device)
    try:
        for t, a in enumerate(tables):
            ctx.upload_table(t, a)
        ctx.set_pooling(hots)
        assert (ctx.pooling_modes == SUM).all()
        wk = fr.Worker(ctx, max(case["batches"]))
        d_dense = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None

        def gather(B, dst, w_shift, kernel):
            ri, pi = _device_rows(fr, ctx, idx[:B])
            rw, pw = _device_rows(fr, ctx, weights[:B], w_shift)
            try:
                wk.gather_pooled(B, pi, d_dense, dst.ptr, weights=pw)
                name = wk.last_kernel()
                wk.sync()
            finally:
                ri.free()
                rw.free()
            if device != CPU:
                assert name == kernel, (name, kernel)

        for B in case["batches"]:
            dst = GM.Guarded(fr, ctx, B, K * 4)
            gather(B, dst, 0, case["kernel"])
            _check_guarded(dst, want[:B], K)
            if case["kernel"].endswith("true>") and B == max(case["batches"]):
                dst.fill()
                gather(B, dst, 4, case["kernel"].replace("true>", "false>"))
                _check_guarded(dst, want[:B], K)
            dst.free()
        wk.close()
    finally:
        ctx.close()


def run_case_modes(fr, device, case_id):
    """Check 2: the case unweighted with every column MEAN and with alternating SUM / MEAN columns.  The case data (gather_matrix.pooled_data)
    holds bags of n = 0, 1 and n = hots non-empty slots in every case, a full bag of two or more slots wherever a column has two, and a bag of
    n = 2 in every case with a column of 2 .. 15 slots: the cases of one-slot bags cannot have one, and the bag lengths 1, 16, 17, 33, 63, 64
    of the <1, 16, false> cases do not happen to (their columns of 16 and more slots lose a fifth of them).  So n = 2 is made: a second
    gather of the first items with one bag per column cut to two slots, in every case and every column that has two slots at all."""
    case, m, tables, hots, idx, dense, _, onehot, want_sum = case_inputs(fr, case_id)
    n = bag_counts(hots, idx)
    assert (n == 0).any() and (n == 1).any() and (n == np.asarray(hots)[None, :]).any()
    assert (n == 2).any() or not any(2 <= int(h) <= 15 for h in hots)
    assert ((n >= 2) & (n == np.asarray(hots)[None, :])).any() or int(max(hots)) < 2
    K = m.record_len
    B = max(case["batches"])
    ctx = fr.Context(m, device=device)
    try:
        for t, a in enumerate(tables):
            ctx.upload_table(t, a)
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, B)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        ri, pi = _device_rows(fr, ctx, idx[:B])
        for modes in (np.full(len(hots), MEAN, np.int32), (np.arange(len(hots)) % 2 == 0).astype(np.int32)):
            ctx.set_pooling_modes(modes)
            assert np.array_equal(ctx.pooling_modes, modes)
            want = expected_modes(fr, m, hots, modes, idx, dense, onehot, sum_records=want_sum)
            assert (want != want_sum).any() or int(max(hots)) < 2
            dst = GM.Guarded(fr, ctx, B, K * 4)
            wk.gather_pooled(B, pi, d_dense, dst.ptr)
            name = wk.last_kernel()
            wk.sync()
            if device != CPU:
                assert name == case["kernel"], (name, case["kernel"])
            _check_guarded(dst, want[:B], K)
            dst.free()
        if int(max(hots)) >= 2:
            # n == 2, the smallest count that divides, in EVERY column of two or more slots (the case's own rows lack it for some bag
            # lengths): the first items again, one bag per column cut to its first and last slot (rows 0 and 6: finite), every column MEAN
            B2 = min(B, 8)
            idx2 = idx[:B2].copy()
            pre = P.prefix_of(hots)
            for c, h in enumerate(hots):
                if h >= 2:
                    idx2[c % B2, pre[c]:pre[c] + int(h)] = -1
                    idx2[c % B2, pre[c]], idx2[c % B2, pre[c] + int(h) - 1] = 0, 6
            n2 = bag_counts(hots, idx2)
            assert all((n2[:, c] == 2).any() for c, h in enumerate(hots) if h >= 2)
            d2 = None if dense is None else dense[:B2]
            modes = np.full(len(hots), MEAN, np.int32)
            ctx.set_pooling_modes(modes)
            want2 = expected_modes(fr, m, hots, modes, idx2, d2, lambda one: GM.expected_records(m, tables, one, d2))
            r2, p2 = _device_rows(fr, ctx, idx2)
            dst = GM.Guarded(fr, ctx, B2, K * 4)
            wk.gather_pooled(B2, p2, d_dense, dst.ptr)
            name = wk.last_kernel()
            wk.sync()
            if device != CPU:
                assert name == case["kernel"], (name, case["kernel"])
            _check_guarded(dst, want2, K)
            dst.free()
            r2.free()
        ctx.set_pooling_modes(None)
        assert (ctx.pooling_modes == SUM).all()
        dst = GM.Guarded(fr, ctx, B, K * 4)
        wk.gather_pooled(B, pi, d_dense, dst.ptr)
        wk.sync()
        _check_guarded(dst, want_sum[:B], K)
        dst.free()
        ri.free()
        wk.close()
    finally:
        ctx.close()


# ---- check 3: identities -----------------------------------------------------------------------------------------------------------------

def check_ones_identity(fr, device, kind, mode, B=70):
    """All weights 1.0f == the unweighted records, bit for bit (FR_FILL_HASH: no NaN row)."""
    m = P.make_model(fr, kind, index_mode=mode, max_rows=3000)
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
        rng = np.random.default_rng(101)
        for hots in (P.spread_hots(m.idx_cols), np.full(m.idx_cols, 4, np.int32)):
            ctx.set_pooling(hots)
            wk = fr.Worker(ctx, B)
            idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.2, empty_bags=6)
            dense = P.dense_for(rng, m, B)
            plain = wk.gather_pooled_records(idx, dense)
            ones = wk.gather_pooled_records(idx, dense, weights=np.ones(idx.shape, np.float32))
            assert np.array_equal(ones, plain), int((ones != plain).sum())
            twos = wk.gather_pooled_records(idx, dense, weights=np.full(idx.shape, 2.0, np.float32))
            assert not np.array_equal(twos, plain)
            wk.close()
    finally:
        ctx.close()


def check_hots1_mean_is_gather_only(fr, device, kind, mode, B=70):
    m = P.make_model(fr, kind, index_mode=mode, max_rows=3000)
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
        rng = np.random.default_rng(103)
        wk = fr.Worker(ctx, B)
        idx = (rng.random((B, m.idx_cols)) * m.index_ranges()[None, :]).astype(np.int32)
        dense = P.dense_for(rng, m, B)
        want = wk.gather_records(idx, dense)
        ctx.set_pooling(np.ones(m.idx_cols, np.int32), modes=np.full(m.idx_cols, MEAN, np.int32))
        assert (ctx.pooling_modes == MEAN).all()
        assert np.array_equal(wk.gather_pooled_records(idx, dense), want)
        wk.close()
    finally:
        ctx.close()


def check_even_odd_known_answers(fr, device, kind, mode, B=90):
    """FR_FILL_EVEN_ODD (even rows 1.0f, odd rows 0.0f), no reference gather.  Weighted, positive weights: every term is w (even slot)
    or +0.0f (odd slot), so a table float is the sequential fp32 sum of the weights of its bag's even slots.  MEAN: (even slots) / n."""
    m = P.make_model(fr, kind, index_mode=mode, max_rows=3000)
    col = P.column_of_float(fr, m)
    tab = col >= 0
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_EVEN_ODD, 0)
        rng = np.random.default_rng(107)
        for hots in (P.spread_hots(m.idx_cols), np.full(m.idx_cols, 8, np.int32)):
            pre = P.prefix_of(hots)
            idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.25, empty_bags=6)
            dense = P.dense_for(rng, m, B)
            w = np.exp2(rng.uniform(-4.0, 2.0, idx.shape)).astype(np.float32)
            w[idx == -1] = np.float32(np.nan)
            acc = np.zeros((B, len(hots)), np.float32)
            even = np.zeros((B, len(hots)), np.float32)
            for c, h in enumerate(hots):
                for j in range(int(h)):
                    s = idx[:, pre[c] + j]
                    e = (s != -1) & (s % 2 == 0)
                    acc[:, c] = np.where(e, np.add(acc[:, c], w[:, pre[c] + j], dtype=np.float32), acc[:, c])
                    even[:, c] += e
            n = bag_counts(hots, idx).astype(np.float32)
            with np.errstate(all="ignore"):
                mean = np.where(n >= 2, np.divide(even, np.maximum(n, 1), dtype=np.float32), even).astype(np.float32)
            ctx.set_pooling(hots)
            wk = fr.Worker(ctx, B)
            for modes, weights, per_col in ((None, w, acc), (np.full(len(hots), MEAN, np.int32), None, mean)):
                ctx.set_pooling_modes(modes)
                want = np.zeros((B, m.record_len), np.float32)
                want[:, tab] = per_col[:, col[tab]]
                want = _with_dense(want.view(np.uint32), col, dense)
                got = wk.gather_pooled_records(idx, dense, weights=weights)
                assert np.array_equal(got, want.ravel()), int((got != want.ravel()).sum())
            wk.close()
    finally:
        ctx.close()


# ---- check 4: scores ---------------------------------------------------------------------------------------------------------------------

def check_scores(fr, device, kind, precision=None, B=48):
    """infer_pooled with weights, and MEAN through infer_pooled: the scores equal fr_worker_fc_only on the EXPECTED records bit for bit (the
    same chain from the same records), and so do the device forms."""
    m = P.make_model(fr, kind, max_rows=3000)
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        if precision is not None:
            ctx.set_fc_precision(precision)
        rng = np.random.default_rng(109)
        hots = P.spread_hots(m.idx_cols)
        idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.2, empty_bags=5)
        dense = P.dense_for(rng, m, B)
        weights = make_weights(rng, hots, idx)
        one_wk = fr.Worker(ctx, B)
        onehot = lambda one: one_wk.gather_records(one, dense).reshape(B, m.record_len)
        want_w = expected_weighted(fr, m, hots, idx, weights, dense, onehot)
        modes = (np.arange(len(hots)) % 2 == 0).astype(np.int32)
        want_m = expected_modes(fr, m, hots, modes, idx, dense, onehot)
        one_wk.close()
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, B)
        d_i = fr.DeviceBuffer.from_numpy(ctx, idx)
        d_w = fr.DeviceBuffer.from_numpy(ctx, weights)
        d_d = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        d_s = fr.DeviceBuffer(ctx, B * 4)
        assert_bits(wk.gather_pooled_records(idx, dense, weights=weights), want_w, "weighted records")
        ref = wk.fc_scores(want_w.view(np.float32))
        assert np.isfinite(ref).all() and len(set(ref.tolist())) > 1
        assert np.array_equal(wk.infer_pooled(idx, dense, weights=weights), ref)
        wk.submit_pooled_device(B, d_i, d_d, d_s, weights=d_w)
        wk.sync()
        assert np.array_equal(d_s.download(np.float32, B), ref)
        assert np.array_equal(wk.pool_weights[:B], weights, equal_nan=True)
        ctx.set_pooling_modes(modes)
        assert_bits(wk.gather_pooled_records(idx, dense), want_m, "mean records")
        ref_m = wk.fc_scores(want_m.view(np.float32))
        assert not np.array_equal(ref_m, ref)
        assert np.array_equal(wk.infer_pooled(idx, dense), ref_m)
        wk.submit_pooled_device(B, d_i, d_d, d_s)
        wk.sync()
        assert np.array_equal(d_s.download(np.float32, B), ref_m)
        wk.close()
    finally:
        ctx.close()


# ---- check 5: errors ---------------------------------------------------------------------------------------------------------------------

def check_errors(fr, device, kind, mode):
    m = P.make_model(fr, kind, index_mode=mode, max_rows=2000)
    ctx = fr.Context(m, device=device)
    L = fr.lib()
    pi = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    cols = m.idx_cols
    B = 16
    try:
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        rng = np.random.default_rng(113)
        sums, means = np.zeros(cols, np.int32), np.full(cols, MEAN, np.int32)
        # modes before pooling
        assert L.fr_ctx_set_pooling_modes(ctx._h, pi(means), cols) == fr.FR_ERR_STATE
        assert L.fr_ctx_set_pooling_modes(ctx._h, None, 0) == fr.FR_ERR_STATE
        wk_old = fr.Worker(ctx, B)
        assert wk_old.pool_weights is None and not L.fr_worker_pool_weights_ptr(wk_old._h)
        hots = np.full(cols, 2, np.int32)
        ctx.set_pooling(hots)
        # a bad mode, a wrong n_cols: nothing changes
        for badv in (2, -1):
            bad = sums.copy()
            bad[cols // 2] = badv
            assert L.fr_ctx_set_pooling_modes(ctx._h, pi(bad), cols) == fr.FR_ERR_INVALID
        assert L.fr_ctx_set_pooling_modes(ctx._h, pi(means), cols + 1) == fr.FR_ERR_INVALID
        assert (ctx.pooling_modes == SUM).all()
        # modes with a batch in flight
        one = (rng.random((B, cols)) * m.index_ranges()[None, :]).astype(np.int32)
        dense = P.dense_for(rng, m, B)
        wk_old.idx[:B] = one
        if wk_old.dense is not None:
            wk_old.dense[:B] = dense
        wk_old.submit(B)
        assert L.fr_ctx_set_pooling_modes(ctx._h, pi(means), cols) == fr.FR_ERR_STATE
        wk_old.sync()
        assert (ctx.pooling_modes == SUM).all()
        # a weighted host submit on a worker older than set_pooling
        assert L.fr_worker_submit_pooled_weighted(wk_old._h, B) == fr.FR_ERR_STATE
        wk = fr.Worker(ctx, B)
        assert wk.pool_weights.shape == (B, 2 * cols)
        idx = P.random_bags(rng, m.index_ranges(), hots, B, empty_share=0.2)
        weights = make_weights(rng, hots, idx)
        d_i = fr.DeviceBuffer.from_numpy(ctx, idx)
        d_w = fr.DeviceBuffer.from_numpy(ctx, weights)
        d_d = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        d_r = fr.DeviceBuffer(ctx, B * m.record_len * 4)
        d_s = fr.DeviceBuffer(ctx, B * 4)
        vp = lambda b: b.ptr if b is not None else None
        # a NULL weights pointer
        assert L.fr_worker_gather_pooled_weighted(wk._h, B, vp(d_i), None, vp(d_d), vp(d_r)) == fr.FR_ERR_INVALID
        assert L.fr_worker_submit_pooled_weighted_device(wk._h, B, vp(d_i), None, vp(d_d), vp(d_s)) == fr.FR_ERR_INVALID
        # weighted calls on a context with a MEAN column (one is enough); the unweighted calls go on working there
        one_mean = sums.copy()
        one_mean[cols - 1] = MEAN
        ctx.set_pooling_modes(one_mean)
        assert np.array_equal(ctx.pooling_modes, one_mean)
        assert L.fr_worker_gather_pooled_weighted(wk._h, B, vp(d_i), vp(d_w), vp(d_d), vp(d_r)) == fr.FR_ERR_STATE
        assert L.fr_worker_submit_pooled_weighted_device(wk._h, B, vp(d_i), vp(d_w), vp(d_d), vp(d_s)) == fr.FR_ERR_STATE
        assert L.fr_worker_submit_pooled_weighted(wk._h, B) == fr.FR_ERR_STATE
        with pytest.raises(fr.FleetRecError) as e:
            wk.infer_pooled(idx, dense, weights=weights)
        assert e.value.status == fr.FR_ERR_STATE
        mean_rec = wk.gather_pooled_records(idx, dense)
        # set_pooling(hots) again resets the modes to SUM
        ctx.set_pooling(hots)
        assert (ctx.pooling_modes == SUM).all()
        assert not np.array_equal(wk.gather_pooled_records(idx, dense), mean_rec)
        # an out-of-range slot under weights: FR_ERR_INDEX_RANGE, the worker stays usable, the next clean gather gives equal bits
        good = wk.gather_pooled_records(idx, dense, weights=weights)
        good_sc = wk.infer_pooled(idx, dense, weights=weights)
        for badv in (int(m.index_ranges()[0]), -2):
            bad = idx.copy()
            bad[3, 1] = badv
            wb = weights.copy()
            wb[3, 1] = 1.0
            with pytest.raises(fr.FleetRecError) as e:
                wk.gather_pooled_records(bad, dense, weights=wb)
            assert e.value.status == fr.FR_ERR_INDEX_RANGE
            with pytest.raises(fr.FleetRecError) as e:
                wk.infer_pooled(bad, dense, weights=wb)
            assert e.value.status == fr.FR_ERR_INDEX_RANGE
            assert_bits(wk.gather_pooled_records(idx, dense, weights=weights), good, "after an index-range error")
            assert np.array_equal(wk.infer_pooled(idx, dense, weights=weights), good_sc)
        # the binding refuses weights of another shape
        with pytest.raises(fr.FleetRecError) as e:
            wk.gather_pooled_records(idx, dense, weights=weights[:, :-1])
        assert e.value.status == fr.FR_ERR_INVALID
        wk.close()
        wk_old.close()
        ctx.set_pooling(None)
        assert (ctx.pooling_modes == SUM).all()
        assert L.fr_ctx_set_pooling_modes(ctx._h, pi(means), cols) == fr.FR_ERR_STATE
    finally:
        ctx.close()


def check_sharded_refuses_modes(fr, device):
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=500)
    ctx = fr.Context(m, device=device, shard_rank=1, n_shards=3)
    try:
        with pytest.raises(fr.FleetRecError) as e:
            ctx.set_pooling_modes(np.zeros(m.idx_cols, np.int32))
        assert e.value.status == fr.FR_ERR_STATE
        with pytest.raises(fr.FleetRecError) as e:
            ctx.set_pooling_modes(None)
        assert e.value.status == fr.FR_ERR_STATE
    finally:
        ctx.close()


# ---- check 6: hosts ----------------------------------------------------------------------------------------------------------------------

def sender_weights(n_items, cols, hots):
    """What fleetrec_sender --hots N --pool weighted sends: 0.25 * (1 + (b + c + 2 j) % 4) for item b, column c, slot j (exact in fp32)."""
    b, c, j = np.meshgrid(np.arange(n_items), np.arange(cols), np.arange(hots), indexing="ij")
    return (0.25 * (1 + (b + c + 2 * j) % 4)).astype(np.float32).reshape(n_items, cols * hots)


def check_server(fr, device, pool, ragged, free_port_block):
    """fleetrec_server --hots 4 --pool P fed by fleetrec_sender --hots 4 [--pool weighted] [--ragged]: Model-A, even/odd tables, all-ones FC
    weights.  A score is the record's sum x H1 x H2 x H3.  weighted: every record float is a sum of multiples of 0.25 (<= 4 of them, each
    <= 1) and the score a multiple of 0.25 far below 2^24 units: exact in fp32 in any order, so the closed form is THE answer.  mean without
    --ragged: n = 4, quarters, exact likewise.  mean --ragged has thirds: equality with the binding on the same rows only."""
    import os
    import re
    import subprocess
    import time
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "gpu-fpga-recommendation-system_amd", "host")
    batch, total, threads, H = 64, 8, 2, 4
    port = free_port_block(threads)
    srv = subprocess.Popen([os.path.join(host, "fleetrec_server"), "--model", "A", "--batch", str(batch), "--threads", str(threads), "--port", str(port),
                            "--total", str(total), "--tables", "evenodd", "--weights", "ones", "--device", str(device), "--hots", str(H), "--pool", pool],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    time.sleep(0.5)
    snd = subprocess.Popen([os.path.join(host, "fleetrec_sender"), "--model", "A", "--batch", str(batch), "--threads", str(threads), "--port", str(port),
                            "--indices", "reference", "--hots", str(H)] + (["--pool", "weighted"] if pool == "weighted" else []) + (["--ragged"] if ragged else []),
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        out, _ = srv.communicate(timeout=300)
        snd.communicate(timeout=60)
    finally:
        for p in (srv, snd):
            if p.poll() is None:
                p.kill()
    out = out.decode()
    assert srv.returncode == 0, out
    assert "processed %d batches" % total in out, out
    rows = re.findall(r"thread \d+ scores:((?: [-0-9.e+]+)+)", out)
    assert rows, out
    m = fr.Model.builtin(fr.MODEL_A)
    T = m.n_tables
    idx = P.sender_rows(5, T, H, ragged)
    w = sender_weights(5, T, H)
    dims = np.array([t.dim for t in m.tables()], dtype=np.float64)
    s = idx.reshape(5, T, H)
    even = (s != -1) & (s % 2 == 0)
    fc = m.fc
    if pool == "weighted":
        per_table = (even * w.reshape(5, T, H).astype(np.float64)).sum(axis=2)
    else:
        n = (s != -1).sum(axis=2)
        per_table = even.sum(axis=2) / np.maximum(n, 1)
    rec_sum = (per_table * dims[None, :]).sum(axis=1)      # FC1's output, every one of its H1 floats
    known = (rec_sum * fc[1] * fc[2] * fc[3]).astype(np.float32)
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_EVEN_ODD, 0)
        ctx.fill_weights(fr.WEIGHTS_ONES, 0)
        ctx.set_pooling(np.full(m.idx_cols, H, np.int32), modes=np.full(m.idx_cols, MEAN, np.int32) if pool == "mean" else None)
        wk = fr.Worker(ctx, 8)
        mine = wk.infer_pooled(idx, weights=w if pool == "weighted" else None)
        wk.close()
    finally:
        ctx.close()
    assert len(set(mine.tolist())) > 1
    exact = pool == "weighted" or not ragged
    if exact:
        # quarters all the way: a layer sums at most max(H) equal multiples of 0.25 (times a power of two), every partial sum below 2^24 units
        assert (rec_sum * 4 == np.round(rec_sum * 4)).all() and float(rec_sum.max()) * 4 * max(fc[1], fc[2], fc[3]) < 2.0 ** 24
        assert np.array_equal(mine, known), (mine, known)
    for r in rows:
        v = np.array([float(x) for x in r.split()], dtype=np.float32)
        assert np.array_equal(v, mine), (v, mine, out)


def check_server_pool_needs_hots(fr):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    host = os.path.join(root, "gpu-fpga-recommendation-system_amd", "host")
    for prog, extra in (("fleetrec_server", ["--device", "-1"]), ("fleetrec_sender", [])):
        p = subprocess.run([os.path.join(host, prog), "--model", "A", "--pool", "weighted"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode != 0 and "--hots" in p.stdout.decode(), p.stdout.decode()
    p = subprocess.run([os.path.join(host, "fleetrec_server"), "--model", "A", "--device", "-1", "--hots", "4", "--pool", "max"], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=60)
    assert p.returncode != 0
    for extra in (["--stream"], ["--shards", "2"]):     # the refusal of tests/pooled_helpers.py, word for word, with --pool as well
        p = subprocess.run([os.path.join(host, "fleetrec_server"), "--model", "A", "--device", "-1", "--hots", "4", "--pool", "weighted"] + extra,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60)
        assert p.returncode != 0 and "not with --stream or --shards" in p.stdout.decode(), p.stdout.decode()

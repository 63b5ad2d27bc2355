"""Streaming pushes of pooled lookups (fr_worker_push_pooled_device, fr_worker_push_pooled_csr_device, fr_worker_push_pooled_device_list,
include/fleetrec_serving.h): the checks, written once for both back-ends (tests/test_cpu_pooled_stream.py, tests/test_gpu_pooled_stream.py).

Bars.  The operand: np.array_equal over the WHOLE region stage 1 reads (pad items and pad k-rows included) against the numpy fold of
tests/gather_matrix.py put through transport() and laid out as the chain's operand; a NaN input stays a NaN (lp_expected / canon).  Scores of a
pushed pooled batch: np.array_equal against fr_worker_submit_pooled*_device + sync of the same batch on a second worker of the same context
(the same stage kernels over the same operand bytes).  One-hot scores between the stage pipeline and the fused kernel: 1e-5 relative, the
figure include/fleetrec.h states for the two summation orders.  Nothing else has a tolerance."""
import ctypes
import functools

import numpy as np
import pytest

import gather_matrix as GM
import pooled_csr as PC
import pooled_helpers as P
import pooled_modes as PM

CPU = -1
SIZES = (1, 3, 32, 33, 257, 64, 2, 300, 31, 5, 256)   # 11 batches: more than the 8 ring slots and the 5 stages; ldm 32 .. 320, ragged and whole
OPERAND_BATCHES = (1, 3, 33, 1029)                    # ldm 32 / 32 / 64 (31 pad items) / 1056; ragged against 1, 2 and 4 items per thread
FORMS = ("sum", "mean", "weighted", "csr", "csr_weighted")


def status_of(fr, fn):
    try:
        fn()
    except fr.FleetRecError as e:
        return e.status
    return fr.FR_OK


def alt_modes(n_cols):
    return (np.arange(n_cols) % 2 == 0).astype(np.int32)


# ---- 1. the operand, byte for byte (GPU) ---------------------------------------------------------------------------------------------------

def operand_model(fr, name):
    if name in ("mixed", "wide"):
        return GM.make_model(fr, name, "table" if name == "wide" else "bank")
    if name == "A":
        return P.make_model(fr, 0, max_rows=20000)
    return P.make_model(fr, 2, index_mode=fr.INDEX_PER_BANK, max_rows=500)   # "C": SEMANTIC, per-bank, dense words, a plan


@functools.lru_cache(maxsize=2)
def _operand_inputs(fr, kernel, model_name):
    m = operand_model(fr, model_name)
    case = dict(id="stream-%s-%s" % (kernel, model_name), batches=OPERAND_BATCHES, hots=GM.POOLED_HOTS[kernel])
    tables, hots, idx, dense = GM.pooled_data(m, case)
    rng = np.random.default_rng(GM.case_seed(case) + 5)
    weights = PM.make_weights(rng, hots, idx, special=tuple(GM.SPECIAL_ROWS))
    onehot = lambda one: GM.expected_records(m, tables, one, dense)
    s = GM.pooled_expected(fr, m, tables, hots, idx, dense)
    want = {"sum": s, "mean": PM.expected_modes(fr, m, hots, alt_modes(len(hots)), idx, dense, onehot, sum_records=s),
            "weighted": PM.expected_weighted(fr, m, hots, idx, weights, dense, onehot)}
    return tables, hots, idx, dense, weights, want


def expected_operand(rec_u32, prec, e_x, ldm):
    """Expected records uint32 [B][K] -> (the operand's bytes uint8 [k_rows][ldm][16], bool mask of the same shape: bytes of a NaN expectation)."""
    B, K = rec_u32.shape
    if prec == 0:
        codes, nan, per, dt = rec_u32, PM.is_nan_bits(rec_u32), 4, np.uint32
    else:
        codes, nan = GM.lp_expected(rec_u32, prec, e_x)
        per, dt = (8, np.uint16) if prec == 1 else (16, np.uint8)
    KP = (K + 63) // 64 * 64 if prec == 2 else K
    assert KP % per == 0
    cp, npad = np.zeros((B, KP), dt), np.zeros((B, KP), bool)
    cp[:, :K], npad[:, :K] = codes, nan
    X, N = np.zeros((KP // per, ldm, per), dt), np.zeros((KP // per, ldm, per), bool)
    X[:, :B], N[:, :B] = cp.reshape(B, KP // per, per).transpose(1, 0, 2), npad.reshape(B, KP // per, per).transpose(1, 0, 2)
    return X, N


def read_operand(fr, ctx, wk, like):
    p = fr.lib().fr_worker_features_dptr(wk._h, None)
    out = np.empty(like.shape, like.dtype)
    fr._check(fr.lib().fr_memcpy_d2h(ctx._h, out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(p), out.nbytes))
    return out


def assert_operand(got, want, nan, prec, exact_nan, what):
    """np.array_equal over the whole region; where the expectation is a NaN the device's code must be a NaN too (fp32 SUM / MEAN: the very bits)."""
    if nan.any() and not exact_nan:
        if prec == 0:
            assert PM.is_nan_bits(got[nan]).all(), "%s: a NaN expectation came back as a number" % what
            got = np.where(nan, want, got)
        else:
            got = GM.canon(got, nan, prec)
    assert np.array_equal(got, want), "%s: %d of %d operand elements differ (first at %s)" % (
        what, int((got != want).sum()), got.size, tuple(int(v[0]) for v in np.nonzero(got != want)))


def check_operand(fr, device, kernel, model_name, prec):
    tables, hots, idx, dense, weights, want = _operand_inputs(fr, kernel, model_name)
    m = operand_model(fr, model_name)
    narrow = kernel.endswith("false>")
    ctx = fr.Context(m, device=device)
    try:
        for t, a in enumerate(tables):
            ctx.upload_table(t, a)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        if prec:
            ctx.set_fc_precision(prec)
        e_x = ctx.fp8_exponents()[0][0] if prec == fr.FC_FP8 else 0
        ctx.set_pooling(hots)
        assert GM.pooled_kernel_for(hots) == kernel
        Bmax = max(OPERAND_BATCHES)
        wk = fr.Worker(ctx, Bmax)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        d_s = fr.DeviceBuffer(ctx, Bmax * 4)
        for form in FORMS:
            if form.startswith("csr") and not narrow:
                continue
            kind = {"csr": "sum", "csr_weighted": "weighted"}.get(form, form)
            ctx.set_pooling_modes(alt_modes(len(hots)) if kind == "mean" else None)
            for B in OPERAND_BATCHES:
                w = weights[:B] if kind == "weighted" else None
                if form.startswith("csr"):
                    off, ind, wf = fr.bags_to_csr(idx[:B], hots, weights=w)
                    c = PC.Csr(fr, ctx, off, ind, wf, (12, 4, 8))
                    wk.push_pooled_csr_device(B, c.off, c.ind, c.nnz, d_dense, d_s, weights=c.w)
                    held = [c.free]
                else:
                    ri, pi = PM._device_rows(fr, ctx, idx[:B])
                    rw, pw = PM._device_rows(fr, ctx, w) if w is not None else (None, None)
                    wk.push_pooled_device(B, pi, d_dense, d_s, weights=pw)
                    held = [ri.free] + ([rw.free] if rw is not None else [])
                name = wk.last_kernel()
                wk.sync()
                for f in held:
                    f()
                assert name == (GM.pooled_kernel_for(hots, aligned=False) if form.startswith("csr") else kernel), (name, kernel, form)
                X, N = expected_operand(want[kind][:B], prec, e_x, (B + 31) // 32 * 32)
                got = read_operand(fr, ctx, wk, X)
                assert_operand(got, X, N, prec, exact_nan=(prec == 0 and kind != "weighted"), what="%s %s B=%d prec=%d" % (kernel, form, B, prec))
        wk.close()
    finally:
        ctx.close()


# ---- 2. scores equal the submit form, bit for bit ---------------------------------------------------------------------------------------------

class Batches:
    """len(SIZES) pooled batches with buffers of their own on the device, in the padded and the offsets form."""

    def __init__(self, fr, ctx, m, caps, rng, sizes=SIZES):
        self.fr, self.ctx, self.sizes = fr, ctx, sizes
        self.rect = [P.random_bags(rng, m.index_ranges(), caps, B, empty_share=0.2, empty_bags=min(5, B)) for B in sizes]
        self.dense = [P.dense_for(rng, m, B) for B in sizes]
        self.w = [PC.csr_weights(rng, r.shape) for r in self.rect]
        self.d_idx = [fr.DeviceBuffer.from_numpy(ctx, r) for r in self.rect]
        self.d_w = [fr.DeviceBuffer.from_numpy(ctx, w) for w in self.w]
        self.d_dense = [fr.DeviceBuffer.from_numpy(ctx, d) if d is not None else None for d in self.dense]
        self.d_s = [fr.DeviceBuffer(ctx, B * 4) for B in sizes]
        self.d_ref = fr.DeviceBuffer(ctx, max(sizes) * 4)
        self.csr = {}
        for weighted in (False, True):
            self.csr[weighted] = [PC.Csr(fr, ctx, *fr.bags_to_csr(r, caps, weights=w if weighted else None), (12, 4, 8)) for r, w in zip(self.rect, self.w)]

    def clear_scores(self):
        for d, B in zip(self.d_s, self.sizes):
            d.upload(np.full(B, np.nan, np.float32))

    def scores(self):
        return [d.download(np.float32, B) for d, B in zip(self.d_s, self.sizes)]

    def push(self, wk, i, form):
        B = self.sizes[i]
        if form.startswith("csr"):
            c = self.csr[form == "csr_weighted"][i]
            wk.push_pooled_csr_device(B, c.off, c.ind, c.nnz, self.d_dense[i], self.d_s[i], weights=c.w)
        else:
            wk.push_pooled_device(B, self.d_idx[i], self.d_dense[i], self.d_s[i], weights=self.d_w[i] if form == "weighted" else None)

    def submit(self, wk, i, form):
        """-> the scores of batch i through the submit form + sync."""
        B = self.sizes[i]
        if form.startswith("csr"):
            c = self.csr[form == "csr_weighted"][i]
            wk.submit_pooled_csr_device(B, c.off, c.ind, c.nnz, self.d_dense[i], self.d_ref, weights=c.w)
        else:
            wk.submit_pooled_device(B, self.d_idx[i], self.d_dense[i], self.d_ref, weights=self.d_w[i] if form == "weighted" else None)
        wk.sync()
        return self.d_ref.download(np.float32, B)


def stream_context(fr, device, kind, precision=None, caps_kind="spread", index_mode=None, max_rows=3000):
    m = P.make_model(fr, kind, index_mode=index_mode, max_rows=max_rows)
    ctx = fr.Context(m, device=device)
    ctx.fill_tables(fr.FILL_HASH, P.SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
    if precision:
        ctx.set_fc_precision(precision)
    caps = P.spread_hots(m.idx_cols) if caps_kind == "spread" else np.ones(m.idx_cols, np.int32) if caps_kind == "ones" else np.full(m.idx_cols, 5, np.int32)
    ctx.set_pooling(caps)
    return m, ctx, caps


def check_scores_equal_submit(fr, device, kind, precision=None, caps_kind="spread", index_mode=None):
    """The 11 batches pushed on one worker without a sync between them, then one sync: every batch's scores equal submit + sync of the same batch
    on a second worker, for SUM, MEAN, weighted and both offsets forms; then the padded forms again through the list call."""
    m, ctx, caps = stream_context(fr, device, kind, precision, caps_kind, index_mode)
    try:
        rng = np.random.default_rng(331)
        wa, wb = fr.Worker(ctx, max(SIZES)), fr.Worker(ctx, max(SIZES))
        bt = Batches(fr, ctx, m, caps, rng)
        seen = {}
        for form in FORMS:
            ctx.set_pooling_modes(alt_modes(len(caps)) if form == "mean" else None)
            ref = [bt.submit(wb, i, form) for i in range(len(SIZES))]
            assert all(np.isfinite(r).all() for r in ref) and len(set(ref[7].tolist())) > 1
            seen[form] = ref
            bt.clear_scores()
            for i in range(len(SIZES)):
                bt.push(wa, i, form)
            wa.sync()
            for i, (g, r) in enumerate(zip(bt.scores(), ref)):
                assert np.array_equal(g, r), "%s: pushed batch %d (%d items) differs from its submit form" % (form, i, SIZES[i])
            if not form.startswith("csr"):
                bt.clear_scores()
                plist = wa.make_pooled_push_list(SIZES, bt.d_idx, bt.d_dense if m.dense_len else None, bt.d_s, weights=bt.d_w if form == "weighted" else None)
                wa.push_pooled_device_list(plist)
                wa.sync()
                for i, (g, r) in enumerate(zip(bt.scores(), ref)):
                    assert np.array_equal(g, r), "%s: listed batch %d (%d items) differs from its submit form" % (form, i, SIZES[i])
        assert np.array_equal(seen["csr"][7], seen["sum"][7]) and np.array_equal(seen["csr_weighted"][7], seen["weighted"][7])
        if int(max(caps)) > 1:
            assert not np.array_equal(seen["sum"][7], seen["mean"][7]) and not np.array_equal(seen["sum"][7], seen["weighted"][7])
        wa.close()
        wb.close()
    finally:
        ctx.close()


# ---- 3. mixing ---------------------------------------------------------------------------------------------------------------------------------

def check_mixing(fr, device, group):
    """One-hot push_device and pooled pushes alternating on one worker, no sync between them.  group 8: both ride the stage pipeline; group None (the
    default, 64, on shrunk Model-A): the one-hot pushes queue for a fused launch and every change of path launches / drains the other."""
    m, ctx, caps = stream_context(fr, device, 0, caps_kind="five")
    try:
        if group:
            ctx.set_stream_group(group)
        rng = np.random.default_rng(337)
        sizes = (64, 33, 256, 5, 70, 64, 1, 31, 128, 7, 40, 40, 40)   # even: one-hot, odd: pooled; the last three: two pooled pushes around a one-hot one
        pooled = [i % 2 == 1 for i in range(len(sizes))]
        pooled[-3:] = [True, False, True]
        wa, wb = fr.Worker(ctx, max(sizes)), fr.Worker(ctx, max(sizes))
        bt = Batches(fr, ctx, m, caps, rng, sizes)
        one = [fr.DeviceBuffer.from_numpy(ctx, (rng.random((B, m.idx_cols)) * m.index_ranges()[None, :]).astype(np.int32)) for B in sizes]
        ref = []
        for i, B in enumerate(sizes):
            if pooled[i]:
                ref.append(bt.submit(wb, i, "sum"))
            else:
                wb.submit_device(B, one[i], bt.d_dense[i], bt.d_ref)
                wb.sync()
                ref.append(bt.d_ref.download(np.float32, B))
        bt.clear_scores()
        for i, B in enumerate(sizes):
            if pooled[i]:
                bt.push(wa, i, "sum")
            else:
                wa.push_device(B, one[i], bt.d_dense[i], bt.d_s[i])
        wa.sync()
        for i, (g, r) in enumerate(zip(bt.scores(), ref)):
            if pooled[i]:
                assert np.array_equal(g, r), "pooled batch %d differs from its submit form" % i
            else:
                assert np.isfinite(g).all() and P.rel_err(g, r) <= 1e-5, "one-hot batch %d: rel err %g" % (i, P.rel_err(g, r))
        wa.close()
        wb.close()
    finally:
        ctx.close()


def check_order_against_update_rows(fr, device):
    """update_rows between two pooled pushes that look up the updated rows, nothing synced in between: the first sees the old rows, the second the new."""
    m = fr.Model.from_spec({"name": "stream_order", "tables": [{"dim": 8, "rows": 3}], "fc": [64, 32, 32]})
    ctx = fr.Context(m, device=device)
    try:
        rng = np.random.default_rng(347)
        old = rng.standard_normal((3, 8)).astype(np.float32)
        new = (old + 100.0).astype(np.float32)
        ctx.upload_table(0, old)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, P.SEED_WEIGHTS)
        ctx.set_pooling(np.array([3], np.int32))
        B = 8
        wa, wb = fr.Worker(ctx, B), fr.Worker(ctx, B)
        rect = P.random_bags(rng, m.index_ranges(), [3], B, empty_share=0.3)
        rect[0] = (0, 1, 2)
        d_idx = fr.DeviceBuffer.from_numpy(ctx, rect)
        d_ids = fr.DeviceBuffer.from_numpy(ctx, np.arange(3, dtype=np.int32))
        d_new = fr.DeviceBuffer.from_numpy(ctx, new)
        s0, s1, sr = (fr.DeviceBuffer(ctx, B * 4) for _ in range(3))
        wb.submit_pooled_device(B, d_idx, None, sr)
        wb.sync()
        ref_old = sr.download(np.float32, B)
        wa.push_pooled_device(B, d_idx, None, s0)
        wa.update_rows(0, 3, d_ids, d_new)
        wa.push_pooled_device(B, d_idx, None, s1)
        wa.sync()
        wb.submit_pooled_device(B, d_idx, None, sr)
        wb.sync()
        ref_new = sr.download(np.float32, B)
        assert not np.array_equal(ref_old, ref_new)
        assert np.array_equal(s0.download(np.float32, B), ref_old)
        assert np.array_equal(s1.download(np.float32, B), ref_new)
        wa.close()
        wb.close()
    finally:
        ctx.close()


# ---- 4. errors and state -------------------------------------------------------------------------------------------------------------------------

def check_range_errors(fr, device):
    """An out-of-range slot in one pushed batch and a malformed offsets bag in another, among clean ones: FR_ERR_INDEX_RANGE at sync, the clean
    batches' scores are right, the worker is usable afterwards."""
    m, ctx, caps = stream_context(fr, device, "spec")
    try:
        rng = np.random.default_rng(349)
        sizes = (33, 7, 64, 5, 12)
        wa, wb = fr.Worker(ctx, max(sizes)), fr.Worker(ctx, max(sizes))
        bt = Batches(fr, ctx, m, caps, rng, sizes)
        ref = [bt.submit(wb, i, "sum") for i in range(len(sizes))]
        bad = bt.rect[1].copy()
        bad[3, 0] = int(m.index_ranges()[0])                       # one past the last row of column 0
        d_bad = fr.DeviceBuffer.from_numpy(ctx, bad)
        off, ind, _ = fr.bags_to_csr(bt.rect[3], caps)
        off = off.copy()
        off[2 * m.idx_cols + 1] = off[2 * m.idx_cols] - 1          # item 2, column 0: end < start
        c_bad = PC.Csr(fr, ctx, off, ind)
        bt.clear_scores()
        bt.push(wa, 0, "sum")
        wa.push_pooled_device(sizes[1], d_bad, bt.d_dense[1], bt.d_s[1])
        bt.push(wa, 2, "csr")
        wa.push_pooled_csr_device(sizes[3], c_bad.off, c_bad.ind, c_bad.nnz, bt.d_dense[3], bt.d_s[3])
        bt.push(wa, 4, "weighted")
        assert status_of(fr, wa.sync) == fr.FR_ERR_INDEX_RANGE
        got = bt.scores()
        for i in (0, 2):
            assert np.array_equal(got[i], ref[i]), "clean batch %d beside a bad one" % i
        assert np.array_equal(got[4], bt.submit(wb, 4, "weighted"))
        keep = np.ones(sizes[1], bool)
        keep[3] = False
        assert np.array_equal(got[1][keep], ref[1][keep])          # every item but the one with the bad slot
        bt.clear_scores()                                          # usable afterwards, and the flag did not stick
        bt.push(wa, 1, "sum")
        bt.push(wa, 3, "csr")
        wa.sync()
        got = bt.scores()
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[3], ref[3])
        c_bad.free()
        wa.close()
        wb.close()
    finally:
        ctx.close()


def check_state_and_arguments(fr, device):
    L = fr.lib()
    m, ctx, caps = stream_context(fr, device, "spec")
    try:
        rng = np.random.default_rng(353)
        B = 9
        wk = fr.Worker(ctx, B)
        bt = Batches(fr, ctx, m, caps, rng, (B,))
        c = bt.csr[False][0]
        ip, wp, dp, sp = (x.ptr if x is not None else None for x in (bt.d_idx[0], bt.d_w[0], bt.d_dense[0], bt.d_s[0]))
        vp = ctypes.c_void_p
        # arguments
        assert L.fr_worker_push_pooled_device(wk._h, B, None, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device(wk._h, B, ip, None, dp, None) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device(wk._h, 0, ip, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device(wk._h, B + 1, ip, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device(None, B, ip, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_csr_device(wk._h, B, None, vp(c.ind), c.nnz, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_csr_device(wk._h, B, vp(c.off), vp(c.ind), -1, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_csr_device(wk._h, B, vp(c.off), None, c.nnz, None, dp, sp) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_csr_device(wk._h, B, vp(c.off), vp(c.ind), c.nnz, None, dp, None) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device_list(wk._h, 1, None, None, None, None, None) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device_list(wk._h, -1, None, None, None, None, None) == fr.FR_ERR_INVALID
        assert L.fr_worker_push_pooled_device_list(wk._h, 0, None, None, None, None, None) == fr.FR_OK
        if m.dense_len:
            assert L.fr_worker_push_pooled_device(wk._h, B, ip, None, None, sp) == fr.FR_ERR_INVALID
        wk.sync()
        # weights with a MEAN column
        ctx.set_pooling_modes(alt_modes(len(caps)))
        assert status_of(fr, lambda: bt.push(wk, 0, "weighted")) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: bt.push(wk, 0, "csr_weighted")) == fr.FR_ERR_STATE
        wk.sync()
        ctx.set_pooling_modes(None)
        # the pooling cannot change under un-synced pushes
        bt.push(wk, 0, "sum")
        assert status_of(fr, lambda: ctx.set_pooling(caps)) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: ctx.set_pooling_modes(alt_modes(len(caps)))) == fr.FR_ERR_STATE
        wk.sync()
        ctx.set_pooling_modes(None)
        # a list stops at its first error: the batches before it stay pushed
        ref = bt.submit(wk, 0, "sum")
        bt.clear_scores()
        plist = wk.make_pooled_push_list((B, B + 1), [bt.d_idx[0]] * 2, [bt.d_dense[0]] * 2 if m.dense_len else None, [bt.d_s[0]] * 2)
        assert status_of(fr, lambda: wk.push_pooled_device_list(plist)) == fr.FR_ERR_INVALID
        wk.sync()
        assert np.array_equal(bt.scores()[0], ref)
        # no pooling set
        ctx.set_pooling(None)
        assert status_of(fr, lambda: bt.push(wk, 0, "sum")) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: bt.push(wk, 0, "csr")) == fr.FR_ERR_STATE
        wk.close()
    finally:
        ctx.close()
    # a BLOCKED-layout context
    mb = P.make_model(fr, 0, layout=fr.LAYOUT_BLOCKED, max_rows=200)
    ctx = fr.Context(mb, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        caps = np.full(mb.idx_cols, 2, np.int32)
        ctx.set_pooling(caps)
        wk = fr.Worker(ctx, 4)
        bt = Batches(fr, ctx, mb, caps, np.random.default_rng(359), (4,))
        assert status_of(fr, lambda: bt.push(wk, 0, "sum")) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: bt.push(wk, 0, "csr")) == fr.FR_ERR_STATE
        assert np.isfinite(bt.submit(wk, 0, "sum")).all()          # (the submit form serves the layout)
        wk.close()
    finally:
        ctx.close()
    # a sharded context
    mc = fr.Model.builtin(fr.MODEL_C).clone(max_rows=500)
    ctx = fr.Context(mc, device=device, shard_rank=1, n_shards=3)
    try:
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        wk = fr.Worker(ctx, 4)
        z = np.zeros(4 * mc.idx_cols + 1, np.int32)
        d_z = fr.DeviceBuffer.from_numpy(ctx, z)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, np.zeros((4, max(mc.dense_len, 1)), np.float32))
        assert status_of(fr, lambda: wk.push_pooled_device(4, d_z, d_dense, d_z)) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: wk.push_pooled_csr_device(4, d_z, None, 0, d_dense, d_z)) == fr.FR_ERR_STATE
        wk.close()
    finally:
        ctx.close()


def check_host_fed_block_refuses(fr, device):
    """Host-fed batches still queued in a block: FR_ERR_STATE ("flush first"), as for fr_worker_update_rows; after the flush the push goes through."""
    m, ctx, caps = stream_context(fr, device, 0, caps_kind="five")
    try:
        rng = np.random.default_rng(367)
        B = 16
        wk, wb = fr.Worker(ctx, B), fr.Worker(ctx, B)
        bt = Batches(fr, ctx, m, caps, rng, (B,))
        ref = bt.submit(wb, 0, "sum")
        host_scores = np.zeros(B, np.float32)
        wk.push_host((rng.random((B, m.idx_cols)) * m.index_ranges()[None, :]).astype(np.int32), bt.dense[0], host_scores)
        assert wk.host_pending()[0] == 1
        assert status_of(fr, lambda: bt.push(wk, 0, "sum")) == fr.FR_ERR_STATE
        wk.flush()
        bt.clear_scores()
        bt.push(wk, 0, "sum")
        wk.sync()
        assert np.array_equal(bt.scores()[0], ref) and np.isfinite(host_scores).all()
        wk.close()
        wb.close()
    finally:
        ctx.close()


def check_cpu_has_no_host_fed_block(fr):
    """Why the refusal above has no CPU case: host-fed streaming is not available on the CPU back-end, so no block can be queued there."""
    m, ctx, caps = stream_context(fr, CPU, "spec")
    try:
        wk = fr.Worker(ctx, 4)
        idx = np.zeros((4, m.idx_cols), np.int32)
        dense = np.zeros((4, m.dense_len), np.float32) if m.dense_len else None
        assert status_of(fr, lambda: wk.push_host(idx, dense, np.zeros(4, np.float32))) == fr.FR_ERR_STATE
        assert status_of(fr, lambda: wk.stage_acquire(4)) == fr.FR_ERR_STATE
        assert wk.host_pending() == (0, 0, 0)
        wk.close()
    finally:
        ctx.close()


# ---- 5. accounting ---------------------------------------------------------------------------------------------------------------------------------

def kernel_records(fr):
    import importlib.util
    import os
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_records(fr.LIB_PATH)

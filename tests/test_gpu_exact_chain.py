"""GPU parity on integer-valued data (tests/exact_chain.py): every FC-chain kernel, through every entry point, bit for bit against the host's
exact restatement of the chain -- no tolerance.  Each case of exact_chain.CASES also pins the kernel the dispatcher picks for it; each
row of exact_chain.SWEEPS runs one kernel at an edge of the shapes its dispatch predicate accepts (test_exact_sweep).  The master-weight side
(end of the module): each reader of a weight image on weights that must round (exact_chain.WIDE), the fp8 exponents taken from the weights,
and a sequence of set_weights / set_fc_precision calls that must each leave every derived image fresh.  The record side after it: each
reader of a record on tables that its conversion must round (exact_chain.RECORDS), preimage rows written by update_rows, calibration on them,
and each fp32 reader on operands that need the whole significand (exact_chain.F32_WIDTH)."""
import numpy as np
import pytest

import exact_chain as E

pytestmark = pytest.mark.gpu


def _prec(fr, p):
    return {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[p]


def _same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s: %d of %d items differ, first %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, np.flatnonzero(bad)[:8].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _setup(fr, gpu, case, batch=None):
    B = batch or case["batch"]
    sp, data, idx, dense = E.case_data(case, B)
    m = fr.Model.from_spec(sp)
    ctx = fr.Context(m, device=gpu)
    E.load(ctx, data)
    ctx.set_fc_precision(_prec(fr, case["prec"]))
    if case.get("width"):
        ctx.set_chain_width(case["width"])
    rec = E.records(m, data, idx, dense)
    return m, ctx, data, idx, dense, rec


def _expect(case, ctx, wk, idx, dense, rec, ws):
    """Premise, rounding witnesses, fp8 calibration -> the exact scores."""
    ae = we = None
    if case["prec"] == "fp8":
        wk.calibrate_fp8(idx, dense)
        ae, we = ctx.fp8_exponents()
        assert we == E.w_exponents(ws), (we, E.w_exponents(ws))
        assert ae == E.act_exponents(rec, ws), (ae, E.act_exponents(rec, ws))
    E.premise(case["prec"], rec, ws, ae, we)
    if case["prec"] != "f32" and rec.shape[0] >= 32:
        for l, (inexact, ties) in enumerate(E.rounding_witnesses(case["prec"], rec, ws, ae, we)):
            assert inexact > 0 and ties > 0, (l, inexact, ties)
    return E.expected(case["prec"], rec, ws, ae, we), ae, we


@pytest.mark.parametrize("case", E.CASES, ids=[c["id"] for c in E.CASES])
def test_exact_case(fr, gpu, case):
    """infer (submit) twice, fc_only, one push and a full stream group of pushes into NaN-filled buffers one ldm long: every item bit-exact,
    nothing written past the batch; the streamed launch's and every layer's kernel as the case names them."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    ldm = (B + 31) // 32 * 32
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(case, ctx, wk, idx, dense, rec, ws)
        _same(wk.infer(idx, dense), want, "infer")
        _same(wk.infer(idx, dense), want, "infer, second run")
        _same(wk.fc_scores(rec), want, "fc_only")
        ctx.set_stream_group(case["group"])
        d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
        d_d = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(dense)) if dense is not None else None
        for n_push in (1, case["group"]):
            outs = []
            for _ in range(n_push):
                o = fr.DeviceBuffer(ctx, ldm * 4)
                o.upload(np.full(ldm, np.nan, np.float32))
                wk.push_device(B, d_i, d_d, o)
                outs.append(o)
            wk.sync()
            if n_push == case["group"] and case.get("stream"):
                assert wk.last_kernel() == case["stream"], wk.last_kernel()
            for j, o in enumerate(outs):
                got = o.download(np.float32, ldm)
                _same(got[:B], want, "push %d of %d" % (j, n_push))
                assert np.isnan(got[B:]).all(), "push %d of %d wrote past the batch" % (j, n_push)
                o.free()
        names = []
        for l in range(4):
            wk.fc_layer_only(B, l)
            names.append(wk.last_kernel())
            wk.sync()
        for l, want_k in enumerate(case.get("layers") or []):
            if want_k:
                assert names[l] == want_k, (l, names)
    finally:
        wk.close()
        ctx.close()


@pytest.mark.parametrize("row", E.SWEEPS, ids=[r["id"] for r in E.SWEEPS])
def test_exact_sweep(fr, gpu, row):
    """A shape on an edge of a kernel's accepted range (exact_chain.SWEEPS): one infer, then one push -- or the row's stream group of pushes,
    where it names a streamed kernel -- into NaN-filled buffers one ldm long: every item bit-exact, nothing written past the batch, and the
    swept layer (or the streamed launch) ran the kernel the row names."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, row)
    B, ws = row["batch"], data["ws"]
    ldm = (B + 31) // 32 * 32
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(row, ctx, wk, idx, dense, rec, ws)
        _same(wk.infer(idx, dense), want, "infer")
        ctx.set_stream_group(row["group"])
        d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
        d_d = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(dense)) if dense is not None else None
        streamed = row["layer"] == "stream"
        n_push = row["group"] if streamed else 1
        outs = []
        for _ in range(n_push):
            o = fr.DeviceBuffer(ctx, ldm * 4)
            o.upload(np.full(ldm, np.nan, np.float32))
            wk.push_device(B, d_i, d_d, o)
            outs.append(o)
        wk.sync()
        if streamed:
            assert wk.last_kernel() == row["kernel"], wk.last_kernel()
        for j, o in enumerate(outs):
            got = o.download(np.float32, ldm)
            _same(got[:B], want, "push %d of %d" % (j, n_push))
            assert np.isnan(got[B:]).all(), "push %d of %d wrote past the batch" % (j, n_push)
            o.free()
        if not streamed:
            wk.fc_layer_only(B, ("FC1", "FC2", "FC3").index(row["layer"]))
            name = wk.last_kernel()
            wk.sync()
            assert name == row["kernel"], name
    finally:
        wk.close()
        ctx.close()


OUT_CASES = [c for c in E.CASES if c.get("gather_out")]


@pytest.mark.parametrize("case", OUT_CASES, ids=[c["id"] for c in OUT_CASES])
def test_exact_gather_out_launch(fr, gpu, case):
    """Five pushes in flight on a chain whose FC layers are GEMM launches and whose output layer is a pipeline stage: the fifth push's step
    is the gather of batch 5 and the output layer of batch 1 in ONE launch, fr_gather_out_kernel<P> (named by the case as a kernel no hook
    reports: pushes on the stage pipeline leave fr_worker_last_kernel alone) -- every score of all five batches bit-exact, nothing written
    past the batch."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    ldm = (B + 31) // 32 * 32
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(case, ctx, wk, idx, dense, rec, ws)
        ctx.set_stream_group(case["group"])
        d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
        d_d = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(dense)) if dense is not None else None
        outs = []
        for _ in range(5):
            o = fr.DeviceBuffer(ctx, ldm * 4)
            o.upload(np.full(ldm, np.nan, np.float32))
            wk.push_device(B, d_i, d_d, o)
            outs.append(o)
        wk.sync()
        for j, o in enumerate(outs):
            got = o.download(np.float32, ldm)
            _same(got[:B], want, "push %d of 5" % j)
            assert np.isnan(got[B:]).all(), "push %d of 5 wrote past the batch" % j
            o.free()
    finally:
        wk.close()
        ctx.close()


NAN_CASES = [c for c in E.CASES if c["id"] in ("bf16-C-4096", "f32-C-4096")]


@pytest.mark.parametrize("case", NAN_CASES, ids=[c["id"] for c in NAN_CASES])
def test_exact_nan_row(fr, gpu, case):
    """A NaN in one table row hit by exactly two items: those two scores are NaN, every other score stays bit-exact (GEMM tiles and, in
    bf16, the fused FC3 + output tail)."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    idx = idx.copy()
    t, r = 0, 0
    idx[idx[:, t] == r, t] = 1
    hit = [5, B - 3]
    idx[hit, t] = r
    rows = data["tables"][t].copy()
    rows[r, 1] = np.nan
    ctx.upload_table(t, rows)
    data = dict(data, tables=[rows] + data["tables"][1:])
    rec = E.records(m, data, idx, dense)
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(case, ctx, wk, idx, dense, rec, ws)
        assert np.flatnonzero(np.isnan(want)).tolist() == hit
        got = wk.infer(idx, dense)
        assert np.flatnonzero(np.isnan(got)).tolist() == hit
        _same(got, want, "infer with a NaN row")
    finally:
        wk.close()
        ctx.close()


def test_exact_fp8_calibration_ignores_stale_padding(fr, gpu):
    """Calibrating on 33 items right after 64 items with larger activations (same ldm of 64): the exponents are those of the 33 items."""
    case = next(c for c in E.CASES if c["id"] == "fp8-C-b65")
    m, ctx, data, _, _, _ = _setup(fr, gpu, case)
    ws = data["ws"]
    pool, dpool = data["idx"], data["dense"]
    acts, _ = E.fp32_acts(E.records(m, data, pool, dpool), ws)
    order = np.argsort(np.abs(acts[1]).max(axis=1))
    big, small = order[-64:], order[:33]
    wk = fr.Worker(ctx, 64)
    try:
        wk.calibrate_fp8(pool[big], dpool[big])
        rec_s = E.records(m, data, pool[small], dpool[small])
        e_big, e_small = E.act_exponents(E.records(m, data, pool[big], dpool[big]), ws), E.act_exponents(rec_s, ws)
        assert ctx.fp8_exponents()[0] == e_big
        assert e_big != e_small          # (else the check below proves nothing)
        wk.calibrate_fp8(pool[small], dpool[small])
        assert ctx.fp8_exponents()[0] == e_small, (ctx.fp8_exponents()[0], e_small)
        _same(wk.infer(pool[small], dpool[small]), E.expected("fp8", rec_s, ws, e_small, E.w_exponents(ws)), "infer after recalibration")
    finally:
        wk.close()
        ctx.close()


EXT_CASES = [c for c in E.CASES if c["id"] in ("fp8-A352", "fp8-B880", "fp8-C-4096", "fp8-C-4096-w4", "fp8-Q-4096-w4", "fp8-K256-4096", "fp8-C-b65",
                                                "fp8-C-1638")]


@pytest.mark.parametrize("shift", [3, -8], ids=["saturate", "subnormal"])
@pytest.mark.parametrize("case", EXT_CASES, ids=[c["id"] for c in EXT_CASES])
def test_exact_fp8_extremes(fr, gpu, case, shift):
    """Activation exponents 3 binades above calibration (values clamp at +-448) or 8 below (e4m3 subnormals and flushes to zero):
    still bit-exact against clamp-then-RNE on every fp8 kernel (fused, 128 x 256 / 256 x 256 / 128 x 128 / 64 x 128 tiles, the FC3 tail,
    the stage pipeline), through submit and a push."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    wk = fr.Worker(ctx, B)
    try:
        wk.calibrate_fp8(idx, dense)
        ae, we = ctx.fp8_exponents()
        ae = [e + shift for e in ae]
        ctx.set_fp8_act_exponents(ae)
        E.premise("fp8", rec, ws, ae, we)
        _, hidden = E.operands("fp8", rec, ws, ae, we)
        if shift > 0:
            assert any((np.abs(r) > 448).any() for r, _ in hidden)
        else:
            assert any(((x != 0) & (np.abs(x) < 2.0 ** -6)).any() for _, x in hidden)
        want = E.expected("fp8", rec, ws, ae, we)
        _same(wk.infer(idx, dense), want, "infer")
        ctx.set_stream_group(case["group"])
        d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
        d_d = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(dense)) if dense is not None else None
        ldm = (B + 31) // 32 * 32
        o = fr.DeviceBuffer(ctx, ldm * 4)
        o.upload(np.full(ldm, np.nan, np.float32))
        wk.push_device(B, d_i, d_d, o)
        wk.sync()
        if case.get("stream"):   # the fused fp8 kernels take the push; the GEMM shapes take the same kernels as in test_exact_case
            assert wk.last_kernel() == case["stream"], wk.last_kernel()
        got = o.download(np.float32, ldm)
        _same(got[:B], want, "push")
        assert np.isnan(got[B:]).all(), "the push wrote past the batch"
    finally:
        wk.close()
        ctx.close()


# ---- the master-weight side: weights that must round, exponents taken from the weights, every refresh of a derived image --------------------

def _unique_items(idx, dense):
    """(first occurrence, inverse) of a batch's distinct items: a batch is drawn from a pool of 256, the host reference runs once per item."""
    key = idx if dense is None else np.hstack([idx, np.ascontiguousarray(dense, np.float32).view(np.int32)])
    _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
    return first, np.asarray(inv).ravel()


def _pushes(fr, ctx, wk, B, idx, dense, want, n_push, what=""):
    ldm = (B + 31) // 32 * 32
    d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
    d_d = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(dense)) if dense is not None else None
    outs = []
    for _ in range(n_push):
        o = fr.DeviceBuffer(ctx, ldm * 4)
        o.upload(np.full(ldm, np.nan, np.float32))
        wk.push_device(B, d_i, d_d, o)
        outs.append(o)
    wk.sync()
    name = wk.last_kernel()
    for j, o in enumerate(outs):
        got = o.download(np.float32, ldm)
        _same(got[:B], want, "%spush %d of %d" % (what, j, n_push))
        assert np.isnan(got[B:]).all(), "%spush %d of %d wrote past the batch" % (what, j, n_push)
        o.free()
    d_i.free()
    if d_d is not None:
        d_d.free()
    return name


@pytest.mark.parametrize("row", E.WIDE, ids=[r["id"] for r in E.WIDE])
def test_exact_wide_weights(fr, gpu, row):
    """A reader of a weight image (exact_chain.WIDE) on weights that the pack kernels must round -- ties to even in both directions, carries,
    near-ties, a flush to zero; per-layer fp8 exponents 3 / 6 / 7 -- or, in the fp8 chain's output layer, on an fp32 Wout that no bf16
    image holds.  Run like a sweep row: one infer, then one push, the row's stream group of pushes (a streamed kernel) or five pushes in
    flight (gather | out) into NaN-filled buffers: every item bit-exact, nothing written past the batch, the named kernel ran."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, row)
    B, ws, prec = row["batch"], data["ws"], row["prec"]
    first, inv = _unique_items(idx, dense)
    wk = fr.Worker(ctx, B)
    try:
        if prec == "fp8" and not row["wout"]:   # the calibration's fp32 chain sums these weights inexactly: its maxima must not sit on a binade edge
            assert E.exponent_margin(E.act_exponent_quotients(rec[first], ws)) > 1e-3
        want_u, ae, we = _expect(row, ctx, wk, idx, dense, rec[first], ws)
        for l in row["wide"]:
            if not (prec == "fp8" and l == 3):
                assert min(E.weight_witnesses(prec, l, ws[l], we)) > 0, (l, E.weight_witnesses(prec, l, ws[l], we))
        if prec == "fp8" and not row["wout"]:
            assert len(set(we)) == 3, we
        want = want_u[inv]
        _same(wk.infer(idx, dense), want, "infer")
        ctx.set_stream_group(row["group"])
        layer = row["layer"]
        name = _pushes(fr, ctx, wk, B, idx, dense, want, row["group"] if layer == "stream" else 5 if layer == "gather_out" else 1)
        if layer == "stream":
            assert name == row["kernel"], name
        elif layer == "stages":
            for l in range(4):
                wk.fc_layer_only(B, l)
                name = wk.last_kernel()
                wk.sync()
                assert name == E.PIPE % (l + 1, E._PI[prec]), (l, name)
        elif layer != "gather_out":
            wk.fc_layer_only(B, ("FC1", "FC2", "FC3", "OUT").index(layer))
            name = wk.last_kernel()
            wk.sync()
            assert name == row["kernel"], name
    finally:
        wk.close()
        ctx.close()


def _tiny(fr, gpu, seed=611):
    K, fc = E.TINY
    sp = E.spec(K, fc, name="tiny_exponents")
    data = E.make_data(sp, seed, n_pool=64, table_max=12)
    m = fr.Model.from_spec(sp)
    return m, fr.Context(m, device=gpu), data


@pytest.mark.parametrize("mx", E.W_EXP_MAXIMA, ids=[t[0] for t in E.W_EXP_MAXIMA])
def test_fp8_weight_exponent_from_the_weights(fr, gpu, mx):
    """set_weights in fp8 mode: w_exp[l] = floor_log2(448 / max|W_l|) for a maximum on and beside the edges of (224, 448], at a power-of-two
    quotient, on a tie, far out in the float range -- at the first element, at the last, and as a negative value, in every layer."""
    _, m_val, by_hand = mx
    m, ctx, data = _tiny(fr, gpu)
    try:
        ctx.set_fc_precision(fr.FC_FP8)
        for l in range(3):
            for place in E.W_EXP_PLACES:
                W, _ = E.layer_with_maximum(data["ws"][l], m_val, place)
                assert E.w_exponent(W) == by_hand
                ctx.set_weights(l, W.ravel())
                assert ctx.fp8_exponents()[1][l] == by_hand, (l, place, ctx.fp8_exponents()[1], by_hand)
    finally:
        ctx.close()


def test_fp8_weight_exponent_zero_layer_and_grid_stride_tail(fr, gpu):
    """An all-zero layer gives w_exp = 0.  One layer of Model-C size (3968 x 2048: stats_kernel's grid-stride loop runs 31 times) with its
    maximum, a negative one, among the last 256 elements."""
    m, ctx, data = _tiny(fr, gpu)
    try:
        ctx.set_fc_precision(fr.FC_FP8)
        ctx.set_weights(1, data["ws"][1].ravel())
        assert ctx.fp8_exponents()[1][1] == 7
        ctx.set_weights(1, np.zeros(data["ws"][1].size, np.float32))
        assert ctx.fp8_exponents()[1][1] == 0
    finally:
        ctx.close()
    K, fc, dl = E.MODELS["C"]
    mC = fr.Model.from_spec(E.spec(K, fc, dense_len=dl, name="exponent_C"))
    ctx = fr.Context(mC, device=gpu)
    try:
        ctx.set_fc_precision(fr.FC_FP8)
        rng = np.random.default_rng(77)
        W = rng.integers(-2, 3, size=K * fc[0]).astype(np.float32)
        for pos in (W.size - 1, W.size - 200):
            V = W.copy()
            V[pos] = -27.0
            assert E.w_exponent(V) == 4 and E.w_exponent(V, use_abs=False) == 7
            ctx.set_weights(0, V)
            assert ctx.fp8_exponents()[1][0] == 4, (pos, ctx.fp8_exponents()[1])
    finally:
        ctx.close()


def test_fp8_nan_weight_never_drives_the_scale(fr, gpu):
    """A NaN right beside a layer's maximum: the layer's exponent is the one computed without it.  The output column that uses the weight
    is NaN for every item (NaN x 0 is NaN), and the next layer sums every column, so every score is NaN; with the NaN taken out again
    every score is back to its exact value."""
    m, ctx, data = _tiny(fr, gpu)
    idx, ws = data["idx"][:33], data["ws"]
    rec = E.records(m, data, idx, None)
    E.load(ctx, data)
    ctx.set_fc_precision(fr.FC_FP8)
    wk = fr.Worker(ctx, 33)
    try:
        wk.calibrate_fp8(idx, None)
        ae, we = ctx.fp8_exponents()
        assert we == E.w_exponents(ws) and ae == E.act_exponents(rec, ws)
        E.premise("fp8", rec, ws, ae, we)
        want = E.expected("fp8", rec, ws, ae, we)
        _same(wk.infer(idx, None), want, "infer")
        for l in range(3):
            W = ws[l] * np.float32(1.0 if l == 1 else 0.5 ** l * 3.0)   # a different maximum, hence exponent, per layer
            flat = W.ravel().copy()
            pos = int(np.argmax(np.abs(flat)))
            nan_at = pos + 1 if pos + 1 < flat.size else pos - 1
            clean = E.w_exponent(flat)
            flat[nan_at] = np.nan
            assert E.w_exponent(flat) == clean and E.w_exponent(flat, skip_nan=False) != clean
            ctx.set_weights(l, flat)
            got_we = ctx.fp8_exponents()[1]
            assert got_we[l] == clean, (l, got_we, clean)
            assert ctx.fp8_exponents()[0] == ae          # calibrated activation exponents stay
            assert np.isnan(wk.infer(idx, None)).all(), l
            ctx.set_weights(l, ws[l].ravel())
            assert ctx.fp8_exponents()[1] == we
            _same(wk.infer(idx, None), want, "infer after the NaN left layer %d" % l)
    finally:
        wk.close()
        ctx.close()


def test_fp8_uncalibrated_activation_exponents(fr, gpu):
    """Before any calibration the activation exponents are the host restatement of the rms estimate (0.58 at the input, times
    sqrt(sum W^2 / H) per layer, 8 rms must fit 448) -- on weight sets whose quotients lie at least 1 % from a power of two, since the
    device adds its block sums of squares with a float atomic, in no fixed order."""
    for seed, scale in ((611, 1.0), (612, 0.37), (613, 5.0)):
        m, ctx, data = _tiny(fr, gpu, seed)
        try:
            ws = [w * np.float32(scale) for w in data["ws"]]
            want, quot = E.estimated_act_exponents(ws, data["fc"])
            assert E.exponent_margin(quot) >= 0.01, (seed, scale, quot)
            ctx.set_fc_precision(fr.FC_FP8)
            for l in range(4):
                ctx.set_weights(l, ws[l].ravel())
            ae, we = ctx.fp8_exponents()
            assert ae == want and we == E.w_exponents(ws), (seed, scale, ae, want, we)
        finally:
            ctx.close()


@pytest.mark.parametrize("shape", list(E.REFRESH_SHAPES))
def test_exact_refresh_sequence(fr, gpu, shape):
    """exact_chain.REFRESH_OPS on one context: set_weights per layer after the precision was chosen, a precision switch after weights were
    set in another precision, fp8 exponents that follow the weights while the calibrated activation exponents stay.  After every step a
    worker that lives through the whole sequence and a fresh one both give the exact scores of the weights now in force (infer, and the
    shape's stream group of pushes), and those differ from the previous step's, so that no stale image can pass."""
    s = E.REFRESH_SHAPES[shape]
    sp, dA, sets = E.refresh_data(shape)
    B = s["batch"]
    m = fr.Model.from_spec(sp)
    ctx = fr.Context(m, device=gpu)
    idx = dA["idx"][:B]
    rec = E.records(m, dA, idx, None)
    E.load(ctx, dA)
    ctx.set_stream_group(s["group"])
    live = fr.Worker(ctx, B)
    prev, ae, calibrated = None, None, False
    try:
        for n, (op, prec, ws, stale) in enumerate(E.refresh_steps(sets)):
            what = "step %d %s: " % (n, op)
            before = ctx.fp8_exponents()
            if op[0] == "prec":
                ctx.set_fc_precision(_prec(fr, prec))
            else:
                ctx.set_weights(op[1], ws[op[1]].ravel())
            we = None
            if prec == "fp8":
                we = E.w_exponents(ws)
                assert ctx.fp8_exponents()[1] == we, (what, ctx.fp8_exponents(), we)
                if op[0] == "prec":   # calibrate on entering fp8: the exponents of the weights now in force
                    live.calibrate_fp8(idx, None)
                    ae = E.act_exponents(rec, ws)
                else:                  # set_weights(1, A * 8): w_exp[1] drops by 3, everything else stays
                    assert we == [before[1][0], before[1][1] - 3, before[1][2]], (what, before, we)
                assert ctx.fp8_exponents()[0] == ae, (what, ctx.fp8_exponents(), ae)
            E.premise(prec, rec, ws, ae, we)
            want = E.expected(prec, rec, ws, ae, we)
            assert prev is None or not np.array_equal(want, prev), what
            for l, old in stale:   # the scores a stale image of layer l would give are other scores
                assert not np.array_equal(E.expected(prec, rec, old, ae, E.w_exponents(old)), want), (what, l)
            fresh = fr.Worker(ctx, B)
            try:
                for who, wk in (("live worker ", live), ("fresh worker ", fresh)):
                    _same(wk.infer(idx, None), want, what + who + "infer")
                    name = _pushes(fr, ctx, wk, B, idx, None, want, s["group"], what + who)
                    if shape == "fused":
                        assert name.startswith("fr_fused_tile"), (what, name)
            finally:
                fresh.close()
            prev = want
    finally:
        live.close()
        ctx.close()


# ---- the record side: records that every converter must round (exact_chain.RECORDS) ----------------------------------------------------------

def _record_ctx(fr, gpu, row, tables="wide"):
    """Context, worker and expectation of a RECORDS row: (m, ctx, wk, data, idx, dense, rec, want, ae).  tables: "wide" = the row's preimages,
    None = none uploaded (a sharded row: fc_from_slices never reads them; the update_rows case uploads its own)."""
    B, prec = row["batch"], row["prec"]
    sp, data, idx, dense = E.case_data(row, B)
    m = fr.Model.from_spec(sp)
    if row.get("bank"):
        m = m.clone(index_mode=fr.INDEX_PER_BANK)
    ctx = fr.Context(m, device=gpu, shard_rank=0, n_shards=2) if row.get("sharded") else fr.Context(m, device=gpu)
    try:
        ws = data["ws"]
        if tables == "wide" and not row.get("sharded"):
            for t, a in enumerate(data["tables"]):
                ctx.upload_table(t, a)
        for l in range(4):
            ctx.set_weights(l, ws[l].ravel())
        ctx.set_fc_precision(_prec(fr, prec))
        ctx.set_chain_width(row["width"])
        rec = E.records(m, data, idx, dense)
        first, inv = _unique_items(idx, dense)
        stock = E.stock_records(m, data, idx)[first]
        ae = ae_s = we = None
        if prec == "fp8":
            ae_s, ae = E.record_row_exponents(row, stock, ws)
            ctx.set_fp8_act_exponents(ae)
            got_ae, we = ctx.fp8_exponents()
            assert got_ae == ae and we == E.w_exponents(ws), (got_ae, ae, we)
        E.premise(prec, rec[first], ws, ae, we)
        wit = E.record_witnesses(prec, rec[first], ae[0] if ae else 0)
        assert all((n > 0) == (k != "above 448" or bool(row.get("clamp"))) for k, n in wit.items()), wit
        want_u = E.expected(prec, rec[first], ws, ae, we)
        assert np.array_equal(want_u, E.expected(prec, stock, ws, ae_s, we) * np.float32(2.0 ** E.REC_S[prec]))   # the stock scores times 2^s
        return m, ctx, fr.Worker(ctx, B), data, idx, dense, rec, want_u[inv], ae
    except BaseException:
        ctx.close()
        raise


@pytest.mark.parametrize("row", E.RECORDS, ids=[r["id"] for r in E.RECORDS])
def test_exact_wide_records(fr, gpu, row):
    """A reader of a record (exact_chain.RECORDS) on tables and dense features that its conversion to bf16 / e4m3 must round -- ties to even in
    both directions, near-ties, carries, signed zeros, in fp8 flushes to zero and (clamp rows) values above 448.  The rounded record is the
    stock integer record times 2^s, so the scores are the stock scores times 2^s, bit for bit.  Run like a weight row: one infer, then one
    push, the row's stream group of pushes or five pushes in flight into NaN-filled buffers; fr_worker_fc_only on the host's records where the
    batch is small or the row asks for it; fc_from_slices on a sharded row.  A streamed or per-bank row runs with the operand-type bank image
    on and off: the image's rows and the in-kernel conversion give the same bits."""
    m, ctx, wk, data, idx, dense, rec, want, ae = _record_ctx(fr, gpu, row)
    B, prec, layer = row["batch"], row["prec"], row["layer"]
    try:
        if row.get("sharded"):
            offs, lens, F = m.shard_plan(2)
            gathered = np.zeros((2, B, F), np.float32)
            for g in range(2):
                gathered[g, :, :lens[g]] = rec[:, offs[g]:offs[g] + lens[g]]
            ldm = (B + 31) // 32 * 32
            d_g = fr.DeviceBuffer.from_numpy(ctx, gathered)
            for item0, n in ((0, B), (64, B - 64 - 3)):
                d_s = fr.DeviceBuffer(ctx, ldm * 4)
                d_s.upload(np.full(ldm, np.nan, np.float32))
                wk.fc_from_slices(B, item0, n, d_g, d_s)
                wk.sync()
                got = d_s.download(np.float32, ldm)
                _same(got[:n], want[item0:item0 + n], "fc_from_slices of items [%d, +%d)" % (item0, n))
                assert np.isnan(got[n:]).all(), "fc_from_slices wrote past its items"
                d_s.free()
            d_g.free()
            return
        ctx.set_stream_group(row["group"])
        for on in ((1, 0) if row.get("bank") or layer == "stream" else (1,)):
            what = "bank image %s: " % ("on" if on else "off")
            ctx.set_lp_bank_image(on)
            _same(wk.infer(idx, dense), want, what + "infer")
            if row.get("bank") and on:
                assert ctx.lp_bank_image_bytes() > 0, "the large-batch gather of a per-bank context did not build the image"
            # (a `stages` row: four pushes before the sync keep several batches in flight, so their steps are the multi-stage launch)
            name = _pushes(fr, ctx, wk, B, idx, dense, want, row["group"] if layer in ("stream", "stages") else 5 if layer == "gather_out" else 1, what)
            if layer == "stream":
                assert name == row["kernel"], name
        if row.get("bank"):
            assert ctx.lp_bank_image_builds() == 1
        if row.get("fc_only") or B <= 256:
            _same(wk.fc_scores(rec), want, "fc_only")
        if layer == "stages":
            for l in range(4):
                wk.fc_layer_only(B, l)
                name = wk.last_kernel()
                wk.sync()
                assert name == E.PIPE % (l + 1, E._PI[prec]), (l, name)
        elif layer not in ("stream", "gather_out"):
            wk.fc_layer_only(B, ("FC1", "FC2", "FC3", "OUT").index(layer))
            name = wk.last_kernel()
            wk.sync()
            assert name == row["kernel"], name
    finally:
        wk.close()
        ctx.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_exact_records_written_by_update_rows(fr, gpu, prec):
    """Preimage rows written into a live operand-type bank image: the context starts on the NEGATED stock rows (times 2^s, exact in the operand
    type), whose scores are the negated expectation (RNE and the clamp are symmetric); fr_ctx_update_rows then writes every row's preimage,
    the image is patched in place (no rebuild) and the next batch is exact."""
    row = next(r for r in E.RECORDS if r["id"] == "rec-%s-image" % prec)
    m, ctx, wk, data, idx, dense, rec, want, ae = _record_ctx(fr, gpu, row, tables=None)
    try:
        neg = np.float32(-(2.0 ** E.REC_S[prec]))
        for t, a in enumerate(data["stock_tables"]):
            ctx.upload_table(t, a * neg)
        neg_dense = data["stock_dense"][data["sel"]] * neg
        _same(wk.infer(idx, neg_dense), -want, "the negated stock rows")
        assert ctx.lp_bank_image_bytes() > 0
        builds = ctx.lp_bank_image_builds()
        for t, a in enumerate(data["tables"]):
            ctx.update_rows(t, np.arange(a.shape[0]), a)
        _same(wk.infer(idx, dense), want, "after update_rows")
        assert ctx.lp_bank_image_builds() == builds, "the update made the next launch rebuild the image"
        _pushes(fr, ctx, wk, row["batch"], idx, dense, want, 1, "after update_rows: ")
    finally:
        wk.close()
        ctx.close()


@pytest.mark.parametrize("row_id", ["rec-fp8-fused_f6", "rec-fp8-stages"])
def test_fp8_calibration_on_wide_records(fr, gpu, row_id):
    """calibrate on records that are not integers: the fp32 chain sums them inexactly, yet its maxima lie far from a power-of-two edge
    (tests/test_exact_chain_cpu.py checks the margin), so the exponents are certain -- the stock ones minus s, those the row sets by hand."""
    row = next(r for r in E.RECORDS if r["id"] == row_id)
    m, ctx, wk, data, idx, dense, rec, want, ae = _record_ctx(fr, gpu, row)
    try:
        assert E.exponent_margin(E.act_exponent_quotients(rec, data["ws"])) > 1e-2
        ctx.set_fp8_act_exponents([0, 0, 0, 0])
        wk.calibrate_fp8(idx, dense)
        assert ctx.fp8_exponents()[0] == ae == E.act_exponents(rec, data["ws"]), (ctx.fp8_exponents(), ae)
        _same(wk.infer(idx, dense), want, "infer after calibration")
    finally:
        wk.close()
        ctx.close()


# ---- fp32 operand width (exact_chain.F32_WIDTH) ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row", E.F32_WIDTH, ids=[r["id"] for r in E.F32_WIDTH])
def test_exact_f32_width(fr, gpu, row):
    """An fp32 reader on operands that need the whole significand: one carrier of 23 or 24 bits per item in the record (operand A of every
    layer in turn) or in W1 (operand B of FC1), or one of W2, W3, Wout times (1 + 2^-j), j >= 12, three runs (operand B of the later
    layers).  Every score is exact and needs more bits than bf16, fp16 or tf32 hold.  Run like a sweep row."""
    m, ctx, data, idx, dense, rec = _setup(fr, gpu, row)
    B, layer = row["batch"], row["layer"]
    first, inv = _unique_items(idx, dense)
    wk = fr.Worker(ctx, B)
    try:
        ctx.set_stream_group(row["group"])
        for what, l, ws in E.f32_runs(row, data):
            if l is not None:
                for k in range(4):
                    ctx.set_weights(k, ws[k].ravel())
            E.premise("f32", rec[first], ws)
            want = E.expected("f32", rec[first], ws)[inv]
            _same(wk.infer(idx, dense), want, what + "infer")
            name = _pushes(fr, ctx, wk, B, idx, dense, want, row["group"] if layer == "stream" else 5 if layer == "gather_out" else 4 if layer == "stages" else 1, what)
            if layer == "stream":
                assert name == row["kernel"], name
            elif layer == "stages":
                for k in range(4):
                    wk.fc_layer_only(B, k)
                    name = wk.last_kernel()
                    wk.sync()
                    assert name == E.PIPE % (k + 1, 0), (k, name)
            elif layer != "gather_out":
                wk.fc_layer_only(B, ("FC1", "FC2", "FC3").index(layer))
                name = wk.last_kernel()
                wk.sync()
                assert name == row["kernel"], name
    finally:
        wk.close()
        ctx.close()

"""GPU parity on integer-valued data (tests/exact_chain.py): every FC-chain kernel, through every entry point, bit for bit against the host's
exact restatement of the chain -- no tolerance.  Each case of exact_chain.CASES also pins the kernel the dispatcher picks for it; each
row of exact_chain.SWEEPS runs one kernel at an edge of the shapes its dispatch predicate accepts (test_exact_sweep)."""
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

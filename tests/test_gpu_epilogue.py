"""Per-layer bias + ReLU (fr_ctx_set_epilogue) on the GPU: every FC-chain kernel that finishes a layer, through every entry point, bit for bit
against the host restatement of the contract (tests/exact_epilogue.py) on integer-valued data -- no tolerance.  Each case of exact_chain.CASES
and each swept row of exact_epilogue.SWEEP_ROWS also pins the kernel the dispatcher picks for a context WITH an epilogue: the case's own GEMM /
stage-pipeline kernels, and for the fused kernels their epilogue forms fr_epi_tile_*_kernel, with the two documented siblings
(exact_epilogue.epilogue_stream_kernel).  Every test fails on a library without fr_ctx_set_epilogue."""
import numpy as np
import pytest

import exact_chain as E
import exact_epilogue as E2
from gpu_helpers import SEED_TABLES, SEED_WEIGHTS, rel_err, uniform_idx

pytestmark = pytest.mark.gpu
RELU = E2.RELU3


def _prec(fr, p):
    return {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[p]


def _same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s: %d of %d items differ, first %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, np.flatnonzero(bad)[:8].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _apply(ctx, bs, acts=RELU):
    for l in range(4):
        ctx.set_epilogue(l, None if bs is None or bs[l] is None else bs[l], "relu" if l < 3 and acts[l] else "none")


def _setup(fr, gpu, case, bsel=(1, 1, 1, 1), acts=RELU):
    B = case["batch"]
    sp, data, idx, dense = E.case_data(case, B)
    _, _, m, bs = E2.case_biases(fr, case)
    bs = [bs[l] if bsel[l] else None for l in range(4)]
    ctx = fr.Context(m, device=gpu)
    E.load(ctx, data)
    ctx.set_fc_precision(_prec(fr, case["prec"]))
    if case.get("width"):
        ctx.set_chain_width(case["width"])
    _apply(ctx, bs, acts)
    return m, ctx, data, idx, dense, E.records(m, data, idx, dense), bs


def _expect(case, ctx, wk, idx, dense, rec, ws, bs, acts=RELU, full=True):
    """fp8 calibration (exponents read back == act_exponents_epi), premise, clip-share cap -> the exact scores."""
    ae = we = None
    if case["prec"] == "fp8":
        wk.calibrate_fp8(idx, dense)
        ae, we = ctx.fp8_exponents()
        assert we == E.w_exponents(ws), (we, E.w_exponents(ws))
        want_ae = E2.act_exponents_epi(rec, ws, bs, acts)
        assert ae == want_ae, (ae, want_ae)
    E2.premise_epi(case["prec"], rec, ws, bs, acts, ae, we)
    if full:
        E2.assert_clip_shares(case["prec"], rec, ws, bs, acts, ae, we)
    return E2.expected_epi(case["prec"], rec, ws, bs, acts, ae, we), ae, we


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


@pytest.mark.parametrize("case", E.CASES, ids=[c["id"] for c in E.CASES])
def test_epilogue_case(fr, gpu, case):
    """Biases on all four layers, ReLU on the three hidden ones: infer twice, fc_only, one push and a full stream group of pushes into NaN-filled
    buffers one ldm long -- every item bit-exact, nothing written past the batch; the streamed launch's kernel is the case's epilogue form (or its
    documented sibling), every layer's kernel the one the case names."""
    m, ctx, data, idx, dense, rec, bs = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(case, ctx, wk, idx, dense, rec, ws, bs)
        _same(wk.infer(idx, dense), want, "infer")
        _same(wk.infer(idx, dense), want, "infer, second run")
        _same(wk.fc_scores(rec), want, "fc_only")
        ctx.set_stream_group(case["group"])
        stream = E2.epilogue_stream_kernel(case, m.record_len)
        for n_push in (1, case["group"]):
            name = _pushes(fr, ctx, wk, B, idx, dense, want, n_push)
            if n_push == case["group"] and stream:
                assert name == stream, (name, stream)
        if case.get("stream") and not stream:   # a record only the persistent bf16 kernel streams: with an epilogue, the stage pipeline
            assert ctx.stream_group() == 1
        names = []
        for l in range(4):
            wk.fc_layer_only(B, l)
            names.append(wk.last_kernel())
            wk.sync()
        for l, want_k in enumerate(case.get("layers") or []):
            if want_k:
                assert names[l] == E2.epilogue_layer_kernel(want_k), (l, names)
    finally:
        wk.close()
        ctx.close()


@pytest.mark.parametrize("row", E2.SWEEP_ROWS, ids=[r["id"] for r in E2.SWEEP_ROWS])
def test_epilogue_sweep(fr, gpu, row):
    """The procedure of test_exact_sweep with the epilogues set: all of the `stage` family (every split-K plan, the padded fp8 / bf16 records), of
    `chunks` (H1 chunk counts 1 and 3 in every fused kernel) and of `tail` (FC3 + output in one launch), the first row per precision of the others."""
    m, ctx, data, idx, dense, rec, bs = _setup(fr, gpu, row)
    B, ws = row["batch"], data["ws"]
    wk = fr.Worker(ctx, B)
    try:
        want, _, _ = _expect(row, ctx, wk, idx, dense, rec, ws, bs)
        _same(wk.infer(idx, dense), want, "infer")
        ctx.set_stream_group(row["group"])
        streamed = row["layer"] == "stream"
        name = _pushes(fr, ctx, wk, B, idx, dense, want, row["group"] if streamed else 1)
        if streamed:
            stream = E2.epilogue_stream_kernel(row, m.record_len)
            if stream:
                assert name == stream, (name, stream)
            else:        # a record the chunked bf16 kernel has no instantiation for: the documented fallback, the stage pipeline (which no hook names)
                assert ctx.stream_group() == 1
        else:
            wk.fc_layer_only(B, ("FC1", "FC2", "FC3").index(row["layer"]))
            name = wk.last_kernel()
            wk.sync()
            assert name == E2.epilogue_layer_kernel(row["kernel"]), name
    finally:
        wk.close()
        ctx.close()


PARTIAL = [c for c in E.CASES if c["id"] in ("f32-A352-g16", "bf16-C-b65", "fp8-C-4096")]
SETTINGS = [("bias only", (1, 1, 1, 1), (0, 0, 0)), ("relu only", (0, 0, 0, 0), RELU), ("relu on layer 1 alone", (0, 0, 0, 0), (0, 1, 0)),
            ("output bias alone", (0, 0, 0, 1), (0, 0, 0))]


@pytest.mark.parametrize("case", PARTIAL, ids=[c["id"] for c in PARTIAL])
def test_epilogue_partial_settings(fr, gpu, case):
    """Bias only; ReLU only; ReLU on layer 1 alone; the output bias alone: each exact through infer and a stream group of pushes.  Then cleared:
    equal to exact_chain.expected, the chain as it was, under the kernel names a context without an epilogue reports."""
    m, ctx, data, idx, dense, rec, bs_all = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    if case["prec"] == "fp8":
        # without ReLU the fp8 chain's R3 spans both signs and is quantised more coarsely (quantum 2^5 in real units here): the premise wants b_3 on
        # that grid, so this test takes the multiple of 256 next to the case's b_3
        bs_all = bs_all[:3] + [np.array([np.rint(bs_all[3][0] / 256.0) * 256.0 or 256.0], np.float32)]
    wk = fr.Worker(ctx, B)
    try:
        ctx.set_stream_group(case["group"])
        for what, bsel, acts in SETTINGS:
            bs = [bs_all[l] if bsel[l] else None for l in range(4)]
            _apply(ctx, bs, acts)
            want, _, _ = _expect(case, ctx, wk, idx, dense, rec, ws, bs, acts, full=False)
            _same(wk.infer(idx, dense), want, what + ": infer")
            _pushes(fr, ctx, wk, B, idx, dense, want, case["group"], what + ": ")
        _apply(ctx, None, (0, 0, 0))
        ae = we = None
        if case["prec"] == "fp8":
            wk.calibrate_fp8(idx, dense)
            ae, we = ctx.fp8_exponents()
            assert ae == E.act_exponents(rec, ws), (ae, E.act_exponents(rec, ws))
        want = E.expected(case["prec"], rec, ws, ae, we)
        _same(wk.infer(idx, dense), want, "cleared: infer")
        name = _pushes(fr, ctx, wk, B, idx, dense, want, case["group"], "cleared: ")
        if case.get("stream"):
            assert name == case["stream"], name
    finally:
        wk.close()
        ctx.close()


NAN_CASES = [c for c in E.CASES if c["id"] in ("f32-A352-g16", "bf16-C-4096", "fp8-A352", "f32-C-b65")]


@pytest.mark.parametrize("case", NAN_CASES, ids=[c["id"] for c in NAN_CASES])
def test_epilogue_nan_item(fr, gpu, case):
    """A NaN in one table row hit by exactly two items (exact_chain's NaN-row construction): those scores stay NaN through three ReLUs, every
    other score is bit-exact."""
    m, ctx, data, idx, dense, rec, bs = _setup(fr, gpu, case)
    B, ws = case["batch"], data["ws"]
    idx = idx.copy()
    t, r = 0, 0
    idx[idx[:, t] == r, t] = 1
    hit = [5, B - 3]
    idx[hit, t] = r
    rec_clean = E.records(m, data, idx, dense)
    rows = data["tables"][t].copy()
    rows[r, 1] = np.nan
    wk = fr.Worker(ctx, B)
    try:
        ae = we = None
        if case["prec"] == "fp8":   # calibrated on the clean rows (a NaN never drives a scale)
            wk.calibrate_fp8(idx, dense)
            ae, we = ctx.fp8_exponents()
            assert ae == E2.act_exponents_epi(rec_clean, ws, bs, RELU)
        ctx.upload_table(t, rows)
        rec = E.records(m, dict(data, tables=[rows] + data["tables"][1:]), idx, dense)
        E2.premise_epi(case["prec"], rec, ws, bs, RELU, ae, we)
        want = E2.expected_epi(case["prec"], rec, ws, bs, RELU, ae, we)
        assert np.flatnonzero(np.isnan(want)).tolist() == hit
        got = wk.infer(idx, dense)
        assert np.flatnonzero(np.isnan(got)).tolist() == hit
        _same(got, want, "infer with a NaN row")
        ctx.set_stream_group(case["group"])
        _pushes(fr, ctx, wk, B, idx, dense, want, case["group"], "NaN row: ")
    finally:
        wk.close()
        ctx.close()


ORACLE_TOL = {"f32": 1e-3, "bf16": 3e-2, "fp8": 0.15}   # the existing bars against the fp64 chain of the master weights (tests/test_gpu_lowprec.py)


@pytest.mark.parametrize("prec", E.PRECS)
def test_epilogue_float_data(fr, gpu, prec):
    """Model-A shapes (record of 352 floats), hash-filled tables, FR_WEIGHTS_UNIFORM, uniform float biases, ReLU, batch 256, through infer and a
    stream group of pushes.  The bars are the project's existing ones, against the references they are set against in tests/test_gpu_lowprec.py:
    exact_chain.OLD_TOL (1e-3 / 5e-3 / 2e-2 of max|ref|) against the float64-accumulating numpy restatement of the chain's OWN arithmetic --
    exact_epilogue.expected_epi: bf16 / e4m3 operands, float64 sums, the epilogue, one rounding per hidden activation -- and ORACLE_TOL (1e-3 /
    3e-2 / 0.15) against the float64 chain of the fp32 master weights.  In fp32 the GPU and the CPU back-end agree to the header's 1e-6 relative."""
    m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=20000)
    rng = np.random.default_rng(11)
    idx = uniform_idx(rng, m.rows(), 256)
    fc = list(m.fc)
    bs = [(rng.random(fc[l + 1]).astype(np.float32) * 2 - 1) / np.float32(np.sqrt(fc[l])) for l in range(4)]
    got = {}
    for dev in (gpu, fr.DEVICE_CPU) if prec == "f32" else (gpu,):
        ctx = fr.Context(m, device=dev)
        try:
            ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
            ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
            ctx.set_fc_precision(_prec(fr, prec))
            _apply(ctx, bs)
            wk = fr.Worker(ctx, 256)
            if prec == "fp8":
                wk.calibrate_fp8(idx)
            if dev == gpu:
                rec = np.ascontiguousarray(wk.gather_records(idx)).reshape(256, -1).view(np.float32)
                ws = [ctx.get_weights(l).reshape(fc[l], fc[l + 1]) for l in range(4)]
                ae, we = ctx.fp8_exponents() if prec == "fp8" else (None, None)
                ref = E2.expected_epi(prec, rec, ws, bs, RELU, ae, we)
                x = rec.astype(np.float64)
                for l in range(3):
                    x = np.maximum(x @ ws[l].astype(np.float64) + bs[l].astype(np.float64), 0.0)
                oracle = (x @ ws[3].astype(np.float64) + float(bs[3][0])).astype(np.float32).ravel()
            got[dev] = wk.infer(idx)
            ctx.set_stream_group(16)
            d_i = fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(idx))
            outs = [fr.DeviceBuffer(ctx, 256 * 4) for _ in range(16)]
            for o in outs:
                wk.push_device(256, d_i, None, o)
            wk.sync()
            streamed = [o.download(np.float32, 256) for o in outs]
            for o in outs + [d_i]:
                o.free()
            if dev == gpu:
                for s in streamed:
                    assert rel_err(s, ref) <= E.OLD_TOL[prec], (prec, rel_err(s, ref))
                    assert rel_err(s, oracle) <= ORACLE_TOL[prec], (prec, rel_err(s, oracle))
            wk.close()
        finally:
            ctx.close()
    err, err_o = rel_err(got[gpu], ref), rel_err(got[gpu], oracle)
    print("float data, %s: max-norm error against the chain's own arithmetic %.3g (bar %.3g), against the master-weight chain %.3g (bar %.3g)" % (
        prec, err, E.OLD_TOL[prec], err_o, ORACLE_TOL[prec]))
    assert err <= E.OLD_TOL[prec], (prec, err)
    assert err_o <= ORACLE_TOL[prec], (prec, err_o)
    if prec == "f32":
        assert rel_err(got[gpu], got[fr.DEVICE_CPU]) <= 1e-6, rel_err(got[gpu], got[fr.DEVICE_CPU])


def test_epilogue_set_after_the_worker_was_created(fr, gpu):
    """A bf16 record only the persistent kernel streams (528 floats), a worker created and used BEFORE the context gets its epilogue: the stream group
    reads 16, then 1; pushes queued after the change ride the stage pipeline and are exact; cleared, the persistent kernel is back."""
    case = next(c for c in E.CASES if c["id"] == "bf16-H528")
    B = case["batch"]
    sp, data, idx, dense = E.case_data(case, B)
    _, _, m, bs = E2.case_biases(fr, case)
    ctx = fr.Context(m, device=gpu)
    E.load(ctx, data)
    ctx.set_fc_precision(fr.FC_BF16)
    ctx.set_stream_group(case["group"])
    rec, ws = E.records(m, data, idx, dense), data["ws"]
    wk = fr.Worker(ctx, B)
    try:
        plain = E.expected("bf16", rec, ws)
        assert ctx.stream_group() == case["group"]
        assert _pushes(fr, ctx, wk, B, idx, dense, plain, case["group"], "before: ") == case["stream"]
        _apply(ctx, bs)
        assert ctx.stream_group() == 1
        want = E2.expected_epi("bf16", rec, ws, bs, RELU)
        _pushes(fr, ctx, wk, B, idx, dense, want, case["group"], "with the epilogue: ")
        _same(wk.infer(idx, dense), want, "infer with the epilogue")
        _apply(ctx, None, (0, 0, 0))
        assert ctx.stream_group() == case["group"]
        assert _pushes(fr, ctx, wk, B, idx, dense, plain, case["group"], "cleared: ") == case["stream"]
    finally:
        wk.close()
        ctx.close()


def _held_tables(m, off, ln):
    return sorted(set(s.src for s in m.segments() if s.kind != 2 and off <= s.rec_offset < off + ln))


def test_epilogue_sharded_staged(fr, gpu):
    """Two shard contexts staged on one GPU, bf16, batch 65, each given the same epilogues by its owner: every rank's scores are bit-identical to
    the unsharded context's (and to the host restatement)."""
    case = next(c for c in E.CASES if c["id"] == "bf16-C-b65")
    m, whole, data, idx, dense, rec, bs = _setup(fr, gpu, case)
    B, ws = 65, data["ws"]
    want = E2.expected_epi("bf16", rec, ws, bs, RELU)
    offs, lens, _ = m.shard_plan(2)
    ctxs, wks, comms = [], [], []
    try:
        w0 = fr.Worker(whole, B)
        _same(w0.infer(idx, dense), want, "unsharded")
        w0.close()
        for g in range(2):
            c = fr.Context(m, device=gpu, shard_rank=g, n_shards=2)
            ctxs.append(c)
            for t in _held_tables(m, offs[g], lens[g]):
                c.upload_table(t, data["tables"][t])
            for l in range(4):
                c.set_weights(l, ws[l].ravel())
            c.set_fc_precision(fr.FC_BF16)
            _apply(c, bs)
            wks.append(fr.Worker(c, B))
        comms = fr.Comm.init_all(ctxs)
        for w in wks:
            w.idx[:B] = idx
            if dense is not None:
                w.dense[:B] = dense
            w.score[:] = np.nan
        for g in range(2):
            wks[g].submit_sharded(comms[g], B)
        for g in reversed(range(2)):
            wks[g].sync()
        for g in range(2):
            _same(wks[g].score[:B], want, "rank %d" % g)
    finally:
        for w in wks:
            w.close()
        for cm in comms:
            cm.close()
        for c in ctxs:
            c.close()
        whole.close()

"""The gather matrix on the MI355X: every kernel instantiation of csrc/fr_gather.hip, named by a case of tests/gather_matrix.py, against the
segment-by-segment numpy statement of the record -- bit for bit (np.array_equal over the whole guarded destination allocation), with the
kernel fr_worker_last_kernel() reports asserted word for word; the bf16 / e4m3 transports on every fp32 class (ties, saturation, +-0,
+-inf, NaN, subnormals) through the narrow kernel, the stream kernel and the operand-type bank image."""
import numpy as np
import pytest

import gather_matrix as G

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_onehot_case(fr, gpu, case):
    """Every batch of the case into a destination with sentinel margins (and pad columns, for a shard's slice), the kernel as the case
    names it; an out-of-range index in item 0 and in the last item: FR_ERR_INDEX_RANGE, every word of every other lookup as the
    reference has it, the next gather clean.  The three `stream0` cases write records of just over 200 MiB (the write-back store form is
    chosen by size alone) and are compared in blocks of 1024 items."""
    times = G.run_onehot(fr, gpu, case)
    print("%s: %s" % (case["id"], ", ".join("batch %d %.1f ms" % (b, 1e3 * t) for b, t in times[:len(case["batches"])])))


@pytest.mark.parametrize("case", G.POOLED_CASES, ids=[c["id"] for c in G.POOLED_CASES])
def test_pooled_case(fr, gpu, case):
    """Batches 1, 2, 3 and 1029 of every window x items form, on a record with an XCD plan, on one below 64 words and (two forms) on one
    wider than a workgroup without a plan; special rows as a bag's lone slot keep their bits; the 16-byte-index forms fall back to the
    narrow form at an index address 4, 8 and 12 bytes past a 16-byte boundary without changing a bit; a slot equal to the row count and
    a slot of -2 are reported and touch no other lookup."""
    G.run_pooled(fr, gpu, case)


def _classes(bits):
    expo, mant = (bits >> 23) & 0xFF, bits & 0x7FFFFF
    return {"nan": (expo == 255) & (mant != 0), "inf": (expo == 255) & (mant == 0), "zero": (expo == 0) & (mant == 0),
            "subnormal": (expo == 0) & (mant != 0), "normal": (expo != 0) & (expo != 255)}


def _same_codes(got, bits, tp, e_x, what):
    want, nan = G.lp_expected(bits, tp, e_x)
    got = G.canon(got, nan, tp)
    if not np.array_equal(got, want):
        bad = got != want
        per = {k: int((bad & v).sum()) for k, v in _classes(bits).items() if (bad & v).any()}
        i = np.flatnonzero(bad.ravel())[:6]
        raise AssertionError("%s: %d of %d codes differ, by class %s; first inputs %s got %s want %s" % (
            what, int(bad.sum()), bad.size, per, [hex(v) for v in bits.ravel()[i]], [hex(v) for v in got.ravel()[i]], [hex(v) for v in want.ravel()[i]]))


LP_FORMS = [(1, 0), (2, -8), (2, 0), (2, 3), (2, 7)]


@pytest.mark.parametrize("form", ["narrow", "stream"])
def test_transport_rounding_exhaustive(fr, gpu, form):
    """Every fp32 pattern (h << 16) | l of gather_matrix.exhaustive_bits() through pack_bf16x2 and through pack_fp8x4 at X exponents -8,
    0, 3 and 7 (set, not calibrated): gather_pack_kernel<8, TP> on the 16-word record of the table alone, gather_pack_stream_kernel on
    512 words of 32 copies of it, each rolled by its table number (so every value meets every word position modulo 16 rows)."""
    exh = G.exhaustive_bits()
    model = {"narrow": "exh16", "stream": "exh512"}[form]
    m = G.make_model(fr, model, "item")
    ctx = fr.Context(m, device=gpu)
    try:
        for t in range(m.n_tables):
            ctx.upload_table(t, np.roll(exh, t, axis=0))
        if form == "stream":
            ctx.gather_groups()
        B = exh.shape[0]
        bits = np.concatenate([np.roll(exh, t, axis=0) for t in range(m.n_tables)], axis=1)
        wk = fr.Worker(ctx, B)
        d_idx = fr.DeviceBuffer.from_numpy(ctx, np.arange(B, dtype=np.int32)[:, None])
        for tp, e_x in LP_FORMS:
            ctx.set_fp8_act_exponents([e_x, 0, 0, 0])
            dst = G.Guarded(fr, ctx, B, m.record_len * G.ESZ[tp])
            wk.gather_slices(B, d_idx, None, dst.ptr, tp)
            name = wk.last_kernel()
            wk.sync()
            assert name == ("gather_pack_kernel<8, %d>" % tp if form == "narrow" else "gather_pack_stream_kernel<4, 2, %d, 16, false>" % tp), name
            got = dst.buf.download(np.uint8, dst.total)
            body = got[dst.pre:dst.total - dst.post].view(G.NP_T[tp]).reshape(B, m.record_len)
            _same_codes(body, bits, tp, e_x, "%s kernel, transport %d, exponent %d" % (form, tp, e_x))
            dst.check(lambda b0, n: body[b0:b0 + n], m.record_len * G.ESZ[tp])     # (the margins)
            dst.free()
        wk.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", ["bf16", "fp8"])
def test_operand_image_rounding_exhaustive(fr, gpu, prec):
    """The same table as the bank rows of a per-bank context on the bf16 / fp8 chain: at batch 8192 the chain's own gather reads the
    operand-type bank image (convert_rows_lp_kernel<1|2>, built by the first such launch) -- and, with the image switched off, the fp32
    rows, converting them itself.  The chain's operand image of a submit (Worker.features) must hold the same codes either way: every
    producer of the type agrees with the gather's transport forms on every fp32 class."""
    exh = G.exhaustive_bits()
    m = G.make_model(fr, "exh256", "bank")
    tp = 1 if prec == "bf16" else 2
    ctx = fr.Context(m, device=gpu)
    try:
        for t in range(m.n_tables):
            ctx.upload_table(t, np.roll(exh, t, axis=0))
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 1)
        ctx.set_fc_precision(fr.FC_BF16 if tp == 1 else fr.FC_FP8)
        B = 8192
        rows = (np.arange(B) % exh.shape[0]).astype(np.int32)
        idx = np.repeat(rows[:, None], m.idx_cols, axis=1)
        bits = np.concatenate([np.roll(exh, t, axis=0)[rows] for t in range(m.n_tables)], axis=1)
        wk = fr.Worker(ctx, B)
        for e_x in ((0,) if tp == 1 else (-8, 0, 3, 7)):
            if tp == 2:
                ctx.set_fp8_act_exponents([e_x, 0, 0, 0])
            for on in (1, 0):
                ctx.set_lp_bank_image(on)
                wk.infer(idx)
                if on:
                    assert ctx.lp_bank_image_bytes() > 0
                feat = wk.features(B, bf16=tp == 1, fp8=tp == 2)[:m.record_len].T
                _same_codes(feat, bits, tp, e_x, "%s operand image, bank image %s, exponent %d" % (prec, "on" if on else "off", e_x))
        wk.close()
    finally:
        ctx.set_lp_bank_image(1)
        ctx.close()

"""Per-layer bias + ReLU on the integer-valued data of tests/exact_chain.py (helpers only; the tests are tests/test_cpu_epilogue.py and
tests/test_gpu_epilogue.py).

The contract (include/fleetrec_serving.h, fr_ctx_set_epilogue): per layer v = (the layer's sum, exactly as without an epilogue) + b[h], ONE fp32
add after the whole K sum, then ReLU (v > 0 ? v : +0, a NaN stays a NaN), then the chain's own rounding of the hidden activation (bf16: RNE;
fp8: x 2^e_act[l + 1], clamp to +-448, RNE to e4m3).  The output layer adds b_3[0] to the finished sum and has no activation.  Biases here are
integers, so on exact_chain's data the chain stays exact in every summation order: no tolerance.

Biases are derived layer by layer from the case's own 256-item pool on the exact fp32 chain: b_l[h] = -rint(median over the pool of the
pre-activation of unit h) + j_h, j_h in {-1, 0, 1} -- about half of every unit's pre-activations are clipped, no unit is dead.  The share of
clipped values per hidden layer is CAPPED to [0.25, 0.75] for every batch of 32 items or more (clip_shares / assert_clip_shares), asserted
before anything is compared.

expected_epi(..., mutant=NAME) restates a WRONG implementation (MUTANTS): test_cpu_epilogue.py shows that each changes the expected scores of
most items on a row where it applies, i.e. that this data would catch it."""
import zlib

import numpy as np

import exact_chain as E
from gpu_helpers import bf16_round, e4m3_decode_table, e4m3_encode

ACT_NONE, ACT_RELU = 0, 1
RELU3 = (ACT_RELU, ACT_RELU, ACT_RELU)
MUTANTS = ("bias_after_relu", "relu_per_partial", "bias_per_partial", "tile_slip_4hk", "tile_slip_8i", "chunk0_bias", "relu_on_output", "drop_b3",
           "bf16_round_before_bias", "fp8_bias_unscaled", "calib_pre_act")


def relu(v):
    """v > 0 ? v : +0.0; a NaN stays a NaN; -0 and negatives become +0."""
    v = np.asarray(v)
    return np.where(np.isnan(v), v, np.where(v > 0, v, np.zeros((), v.dtype)))


def _e4m3(v):
    """float32 -> the e4m3 value (float64) the device stores: clamp to +-448, RNE; a NaN stays a NaN (the device's compares keep it, the conversion
    encodes it as 0x7F) -- gpu_helpers.e4m3_encode has no NaN code, so it is carried around the helper here."""
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    out = e4m3_decode_table()[e4m3_encode(np.where(nan, np.float32(0), v))]
    out[nan] = np.nan
    return out


def _act(v, a):
    return relu(v) if a == ACT_RELU else v


def make_biases(pool_rec, ws, seed, acts=RELU3):
    """Integer biases b_0..b_3 (float32) from the pool's exact fp32 chain: b_l = -rint(median of pre_l over the pool) + j, j in {-1, 0, 1};
    b_3 = a nonzero integer."""
    rng = np.random.default_rng(seed)
    x = np.asarray(pool_rec, np.float64)
    bs = []
    for l in range(3):
        pre = x @ ws[l].astype(np.float64)
        b = -np.rint(np.median(pre, axis=0)) + rng.integers(-1, 2, size=pre.shape[1])
        bs.append(b.astype(np.float32))
        x = _act(pre + b, acts[l])
    # b_3 puts about two thirds of the pool's scores below zero, so that a (wrong) ReLU on the output layer would show on most items
    b3 = -np.rint(np.quantile(x @ ws[3].astype(np.float64), 0.67)) + float(rng.integers(-1, 2))
    bs.append(np.array([b3 if b3 != 0 else 1.0], np.float32))
    return bs


def case_biases(fr, case, acts=RELU3, jitter=0):
    """(spec, data, model, biases) of a CASES entry or a SWEEPS row: the biases come from the row's own pool; `jitter` re-seeds them (a row whose
    data misses the clip-share cap takes another jitter, never another cap)."""
    sp, data, _, _ = E.case_data(case, 1)
    m = fr.Model.from_spec(sp)
    pool = E.records(m, data, data["idx"], data["dense"])
    return sp, data, m, make_biases(pool, data["ws"], 31000 + zlib.crc32(case["id"].encode()) % 100000 + 7919 * jitter, acts)


def _halves(K):
    """The stage pipeline's split-K plan of two: workgroup 0 takes the first ceil(K / 8 / 2) groups of 8 k (fr_pipeline.hip fc_q_body)."""
    g = K // 8
    return 8 * ((g + 1) // 2)


def _bias_index(N, mutant, layer):
    """The index a (mutant) kernel reads the bias of output n at."""
    n = np.arange(N)
    if mutant == "tile_slip_4hk":
        return n - 4 * ((n >> 2) & 1)
    if mutant == "tile_slip_8i":
        return (n // 32) * 32 + (n % 8)
    if mutant == "chunk0_bias" and layer == 0:
        return n % 256
    return n


def _layer_v(pre_parts, b, act, mutant, layer):
    """fp32 v of one hidden layer from its exact partial sums (float64 [B][N] each; one part unless the layer is split)."""
    f32 = np.float32
    if b is None:
        b = np.zeros(pre_parts[0].shape[1], f32)
    b = np.asarray(b, f32)[_bias_index(b.size, mutant, layer)]
    if mutant == "relu_per_partial" and len(pre_parts) == 2:
        return _act(sum(_act(p.astype(f32), act) for p in pre_parts) + b, act)
    if mutant == "bias_per_partial" and len(pre_parts) == 2:
        return _act(sum(p.astype(f32) + b for p in pre_parts), act)
    pre = sum(pre_parts).astype(f32)
    if mutant == "bias_after_relu":
        return _act(pre, act) + b
    return _act(pre + b, act)


def _split_parts(x, W, nsplit):
    if nsplit == 2:
        h = _halves(W.shape[0])
        return [x[:, :h] @ W[:h], x[:, h:] @ W[h:]]
    return [x @ W]


def chain_epi(prec, rec, ws, bs, acts, act_exp=None, w_exp=None, mutant=None, split=(1, 1, 1)):
    """-> (scores float32 [B], per hidden layer the fp32 v before the chain's rounding, per hidden layer the next layer's operand).  bs[l] may be
    None (no bias); split: the fp32 stage pipeline's split-K plan (only the two split mutants look at it)."""
    f32 = np.float32
    bs = list(bs) if bs is not None else [None] * 4
    vs, xs = [], []
    if prec == "fp8":
        dec = e4m3_decode_table()
        x = _e4m3(np.asarray(rec, f32) * f32(2.0 ** act_exp[0]))
        for l in range(3):
            Wf = dec[e4m3_encode(ws[l] * f32(2.0 ** w_exp[l]))]
            unit = 2.0 ** -(act_exp[l] + w_exp[l])
            if mutant == "fp8_bias_unscaled" and bs[l] is not None:
                v = _act(((x @ Wf + np.asarray(bs[l], np.float64)) * unit).astype(f32), acts[l])
            else:
                v = _layer_v([(x @ Wf) * unit], bs[l], acts[l], mutant, l)
            vs.append(v)
            x = _e4m3(v * f32(2.0 ** act_exp[l + 1]))
            xs.append(x)
        s = ((x * 2.0 ** -act_exp[3]) @ ws[3].astype(np.float64)).astype(f32).ravel()
    else:
        rnd = (lambda v: v) if prec == "f32" else bf16_round
        x = rnd(np.asarray(rec, f32)).astype(np.float64)
        for l in range(3):
            W = rnd(ws[l]).astype(np.float64)
            if mutant == "bf16_round_before_bias" and prec == "bf16":
                parts = [bf16_round((x @ W).astype(f32)).astype(np.float64)]
            else:
                parts = _split_parts(x, W, split[l] if prec == "f32" else 1)
            v = _layer_v(parts, bs[l], acts[l], mutant, l)
            vs.append(v)
            x = rnd(v).astype(np.float64)
            xs.append(x)
        s = (x @ rnd(ws[3]).astype(np.float64)).astype(f32).ravel()
    if bs[3] is not None and mutant != "drop_b3":
        s = s + f32(np.asarray(bs[3], f32).ravel()[0])
    if mutant == "relu_on_output":
        s = relu(s)
    return s.astype(f32), vs, xs


def expected_epi(prec, rec, ws, bs, acts, act_exp=None, w_exp=None, mutant=None, split=(1, 1, 1)):
    """The exact scores float32 [B] of the chain with the epilogues (bs, acts) in precision `prec`."""
    return chain_epi(prec, rec, ws, bs, acts, act_exp, w_exp, mutant, split)[0]


def act_exponents_epi(rec, ws, bs, acts, mutant=None):
    """Calibrated activation exponents floor_log2(448 / (2 max|.|)) of X and the POST-activation R1..R3 of the fp32 chain with the epilogues
    (mutant calib_pre_act: the maxima of the sums before bias and activation)."""
    rec = np.asarray(rec, np.float32)
    _, vs, _ = chain_epi("f32", rec, ws, bs, acts)
    tens = [rec] + vs
    if mutant == "calib_pre_act":
        x, tens = rec.astype(np.float64), [rec]
        for l in range(3):
            tens.append(x @ ws[l].astype(np.float64))
            x = vs[l].astype(np.float64)
    return [E.floor_log2_f32(np.float32(448.0) / (np.float32(2.0) * np.float32(np.abs(a).max()))) for a in tens]


def act_exponent_margin(rec, ws, bs, acts):
    _, vs, _ = chain_epi("f32", np.asarray(rec, np.float32), ws, bs, acts)
    return E.exponent_margin([448.0 / (2.0 * float(np.abs(a).max())) for a in [np.asarray(rec, np.float32)] + vs])


def operands_epi(prec, rec, ws, bs, acts, act_exp=None, w_exp=None):
    """Per layer (A [B][K], W [K][N], b [N] or None) in the domain the device sums in (fp8: real units), post-activation operands."""
    f32 = np.float32
    _, _, xs = chain_epi(prec, rec, ws, bs, acts, act_exp, w_exp)
    bs = list(bs) if bs is not None else [None] * 4
    if prec == "fp8":
        dec = e4m3_decode_table()
        ins = [_e4m3(np.asarray(rec, f32) * f32(2.0 ** act_exp[0])) * 2.0 ** -act_exp[0]] + [x * 2.0 ** -act_exp[l + 1] for l, x in enumerate(xs)]
        Ws = [dec[e4m3_encode(ws[l] * f32(2.0 ** w_exp[l]))] * 2.0 ** -w_exp[l] for l in range(3)] + [ws[3].astype(np.float64)]
    else:
        rnd = (lambda v: v) if prec == "f32" else bf16_round
        ins = [rnd(np.asarray(rec, f32)).astype(np.float64)] + xs
        Ws = [rnd(w).astype(np.float64) for w in ws]
    return [(ins[l], Ws[l], None if bs[l] is None else np.asarray(bs[l], np.float64)) for l in range(4)]


def premise_epi(prec, rec, ws, bs, acts, act_exp=None, w_exp=None):
    """exact_chain.premise on the post-activation operands, plus per layer: sum of |products| + |b| < 2^24 q and b a multiple of q, so the one
    fp32 add of the bias is exact too.  Items with a non-finite feature are left out.  -> per layer (log2 q, worst / (2^24 q))."""
    rec = np.asarray(rec, np.float32)
    live = np.isfinite(rec).all(axis=1)
    out = []
    for l, (A, W, b) in enumerate(operands_epi(prec, rec[live], ws, bs, acts, act_exp, w_exp)):
        la, lw = E._lowbit(A), E._lowbit(W)
        if la is None or lw is None:
            out.append((None, 0.0))
            continue
        q = 2.0 ** (la + lw)
        worst = (np.abs(A) @ np.abs(W)).max(axis=0)
        if b is not None:
            assert (np.mod(b, q) == 0).all(), "layer %d (%s): a bias is no multiple of 2^%d" % (l, prec, la + lw)
            worst = worst + np.abs(b)
        worst = float(worst.max())
        assert worst < 2.0 ** 24 * q, "layer %d (%s): sum of |products| + |b| %g >= 2^24 * 2^%d" % (l, prec, worst, la + lw)
        out.append((la + lw, worst / (2.0 ** 24 * q)))
    return out


def clip_shares(prec, rec, ws, bs, acts, act_exp=None, w_exp=None):
    """Share of v <= 0 per hidden layer, in the precision's own host reference (items with a non-finite feature left out)."""
    rec = np.asarray(rec, np.float32)
    live = np.isfinite(rec).all(axis=1)
    _, vs, _ = chain_epi(prec, rec[live], ws, bs, acts, act_exp, w_exp)
    return [float((v <= 0).mean()) for v in vs]


def assert_clip_shares(prec, rec, ws, bs, acts, act_exp=None, w_exp=None):
    """The cap: for a batch of 32 items or more, the share of v <= 0 at each hidden layer lies in [0.25, 0.75]."""
    if np.asarray(rec).shape[0] < 32:
        return None
    sh = clip_shares(prec, rec, ws, bs, acts, act_exp, w_exp)
    assert all(0.25 <= s <= 0.75 for s in sh), (prec, sh)
    return sh


# the swept rows the epilogue tests run: every `stage`, `chunks` and `tail` row, the first row of the six other families per precision
def sweep_rows():
    rows, seen = [], set()
    for r in E.SWEEPS:
        if r["family"] in ("stage", "chunks", "tail"):
            rows.append(r)
        elif (r["family"], r["prec"]) not in seen:
            seen.add((r["family"], r["prec"]))
            rows.append(r)
    return rows


SWEEP_ROWS = sweep_rows()

# What the streamed launch of a context WITH an epilogue reports.  The fused kernels have an epilogue form under a name of
# its own, fr_epi_tile_*_kernel<same arguments> -- the existing instantiations are compiled as they were -- with two documented siblings:
#   * fr_fused_tile_kernel<2, 44, 4, false> (Model-A fp32, two workgroups per CU in 128 registers): the epilogue form would spill, so such a context
#     takes the one-workgroup-per-CU instantiation <2, 44, 2, true>;
#   * fr_fused_tile_hs_kernel (persistent bf16: 128 accumulators in a budget of 168 registers) has no epilogue form: the launch takes the chunked
#     bf16 kernel where that has an instantiation for the record (K = 352 / 880), the stage pipeline otherwise.
# The GEMM kernels, the stage pipeline and fr_gather_out_kernel have epilogue forms too, same template arguments: fc_epi_*_kernel, fr_epi_pipeline_kernel,
# fr_epi_gather_out_kernel (epilogue_layer_kernel).  All epilogue forms live in libfleetrec_epi.so; libfleetrec.so's kernels carry no epilogue code.
H_KERNEL = {352: "fr_epi_tile_h_kernel<2, 2, 22, true, 16, 2>", 880: "fr_epi_tile_h_kernel<2, 2, 55, false, 12, 2>"}
EPI_NAMES = (("fr_fused_tile_kernel<2, 44, 4, false>", "fr_epi_tile_kernel<2, 44, 2, true>"), ("fr_fused_tile_kernel<", "fr_epi_tile_kernel<"),
             ("fr_fused_tile_m2_kernel<", "fr_epi_tile_m2_kernel<"), ("fr_fused_tile_h_kernel<", "fr_epi_tile_h_kernel<"),
             ("fr_fused_tile_f8_kernel<", "fr_epi_tile_f8_kernel<"))


def epilogue_layer_kernel(name):
    """What fc_layer_only reports for a layer of a context with an epilogue, given the name a context without one reports."""
    if not name:
        return name
    if name.startswith("fc_"):
        return "fc_epi_" + name[3:]
    return name.replace("fr_pipeline_kernel", "fr_epi_pipeline_kernel").replace("fr_gather_out_kernel", "fr_epi_gather_out_kernel")


def epilogue_stream_kernel(case, K):
    """The kernel the streamed launch of a case / row reports when its context has an epilogue (None: the stage pipeline, which no hook names)."""
    name = case.get("stream") if "stream" in case else (case["kernel"] if case.get("layer") == "stream" else None)
    if not name:
        return None
    if "fr_fused_tile_hs_kernel" in name:
        return H_KERNEL.get(K)
    for old, new in EPI_NAMES:
        if name.startswith(old):
            return new + name[len(old):] if old.endswith("<") else new
    return name

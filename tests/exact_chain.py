"""Integer-valued FC-chain data on which every kernel must match the host bit for bit (helpers only; the tests are
tests/test_exact_chain_cpu.py and tests/test_gpu_exact_chain.py).

Tables and dense features are integers in [-3, 3], weights integers in {-2 .. 2}, sparse enough that no layer's sum of |products|
reaches 2^24 times the products' common power-of-two quantum (premise(), asserted before any comparison).  Every fp32 partial sum is
then exact in any order and any split, bf16 / e4m3 products are exact in fp32, the fp8 scales are powers of two: the only roundings
left are the chain's explicit ones (bf16 RNE per hidden layer; e4m3 clamp to +-448 then RNE), which the host restates
(gpu_helpers.chain_bf16_reference / chain_fp8_reference).  So there is no tolerance: one wrong column, k-group or tile shows.
(A sweep row with a record too short for FC1's sums to pass 256 draws its tables from [-12, 12], so that bf16 still rounds there.)
The integer weights are exact in every operand type, so the master-weight side has data of its own: WIDE (weights the pack kernels must
round, an fp32 Wout no bf16 image holds), W_EXP_MAXIMA (fp8 weight exponents read back) and REFRESH_OPS (every refresh of a derived image).
So has the record side: RECORDS (tables and dense features drawn from the preimages of the stock operand images, so that every converter of
a record must round) and F32_WIDTH (fp32 rows whose operands need the whole 24-bit significand), both at the end of the module."""
import re
import zlib

import numpy as np

from gpu_helpers import bf16_round, chain_bf16_reference, chain_fp8_reference, e4m3_decode_table, e4m3_encode

PRECS = ("f32", "bf16", "fp8")
OLD_TOL = {"f32": 1e-3, "bf16": 5e-3, "fp8": 2e-2}   # the max-norm bars the score tests hold the chains to (gpu_helpers, test_gpu_lowprec)
_DIMS = (32, 16, 64, 8, 128, 4)


def spec(K, fc, dense_len=0, rows=29, name=None):
    """A Model.from_spec dict with a K-float record: tables of mixed widths (+ a dense block in the middle), few rows each."""
    dims, left, i = [], K - dense_len, 0
    while left > 0:
        d = _DIMS[i % len(_DIMS)]
        i += 1
        if d <= left:
            dims.append(d)
            left -= d
    return {"name": name or "exact_%d" % K, "tables": [{"dim": d, "rows": rows + 3 * t} for t, d in enumerate(dims)], "dense_len": dense_len,
            "dense_at": len(dims) // 2, "fc": list(fc)}


def _sparse_layer(rng, K, N, nnz, positive=False):
    """K x N integer weights ([k][n]): every row and every column has a nonzero, each column about `nnz` of them, |w| = 2 somewhere."""
    W = np.zeros((K, N), np.float32)
    vals = np.array([-2, -1, 1, 2], np.float32)
    p = [0.05, 0.05, 0.2, 0.7] if positive else None
    rows = rng.permutation(K)
    cols = rng.permutation(N)
    for i in range(max(K, N)):                       # cover every row and every column
        W[rows[i % K], cols[i % N]] = rng.choice(vals, p=p)
    extra = max(nnz - max(K, N) // N, 0)
    if extra:
        kk = rng.integers(0, K, size=(extra, N))
        W[kk, np.arange(N)[None, :]] = rng.choice(vals, size=(extra, N), p=p)
    W[rows[0], cols[0]] = 2.0
    return W


def make_data(model_spec, seed, n_pool=256, table_max=3, nnz=(320, 8, 8)):
    """-> dict: tables (list of float32 [rows][dim]), ws (4 float32 [K][N] arrays, == column-major N x K flattened), fc, and a pool
    of n_pool items (idx int32 [n][n_tables], dense float32 [n][dense_len] or None).  table_max: table and dense values are integers in
    [-table_max, table_max] (3: the stock distribution; a short record takes a wider range so that its FC1 sums pass 256 and bf16 rounds);
    nnz: nonzeros per column of W1, W2, W3 (320, 8, 8: the stock counts; the fp32-Wout rows of WIDE take fewer, see there)."""
    rng = np.random.default_rng(seed)
    fc = [sum(t["dim"] for t in model_spec["tables"]) + model_spec.get("dense_len", 0)] + list(model_spec["fc"]) + [1]
    vals = np.arange(-3, 4, dtype=np.float32)
    pv = np.array([0.02, 0.03, 0.05, 0.1, 0.2, 0.25, 0.35])   # mostly positive: FC1 sums of several hundred (bf16 / e4m3 must round)
    if table_max != 3:   # the same shape stretched: a ramp that favours the positive end
        vals = np.arange(-table_max, table_max + 1, dtype=np.float32)
        pv = np.linspace(1.0, 12.0, vals.size) ** 2
        pv /= pv.sum()
    tables = [rng.choice(vals, size=(t["rows"], t["dim"]), p=pv).astype(np.float32) for t in model_spec["tables"]]
    ws = [_sparse_layer(rng, fc[0], fc[1], min(fc[0], nnz[0]), positive=True), _sparse_layer(rng, fc[1], fc[2], nnz[1]),
          _sparse_layer(rng, fc[2], fc[3], nnz[2]), _sparse_layer(rng, fc[3], 1, 12)]
    rows = np.array([t["rows"] for t in model_spec["tables"]])
    idx = (rng.random((n_pool, len(rows))) * rows[None, :]).astype(np.int32)
    dl = model_spec.get("dense_len", 0)
    dense = rng.choice(vals, size=(n_pool, dl), p=pv).astype(np.float32) if dl else None
    return {"tables": tables, "ws": ws, "fc": fc, "idx": idx, "dense": dense, "spec": model_spec}


def records(model, data, idx, dense=None):
    """The gathered records float32 [B][K] of these rows, from the model's segments (tables + dense block)."""
    idx = np.asarray(idx)
    out = np.empty((idx.shape[0], model.record_len), np.float32)
    for sg in model.segments():
        if sg.kind == 2:   # SEG_DENSE
            out[:, sg.rec_offset:sg.rec_offset + sg.len] = dense[:, sg.src_col:sg.src_col + sg.len]
        else:
            out[:, sg.rec_offset:sg.rec_offset + sg.len] = data["tables"][sg.src][idx[:, sg.src], sg.src_col:sg.src_col + sg.len]
    return out


def load(ctx, data):
    for t, a in enumerate(data["tables"]):
        ctx.upload_table(t, a)
    for l in range(4):
        ctx.set_weights(l, data["ws"][l].ravel())


def floor_log2_f32(v):
    """floor(log2(v)) of a float32 value, the way the library takes it (frexp of the float32 quotient)."""
    return int(np.frexp(np.float32(v))[1]) - 1


def fp32_acts(rec, ws):
    """The fp32 chain's activations X, R1, R2, R3 and its scores, exact (fp64 sums of integers)."""
    acts = [np.asarray(rec, np.float64)]
    for l in range(3):
        acts.append(acts[-1] @ ws[l].astype(np.float64))
    return acts, (acts[-1] @ ws[3].astype(np.float64)).astype(np.float32).ravel()


def w_exponent(W, use_abs=True, skip_nan=True):
    """One layer's fp8 weight exponent floor_log2(448 / max|W|) in float32, the maximum taken over the values that are not NaN; 0 for an
    all-zero layer.  (use_abs / skip_nan False: the mutants `max taken without abs`, whose maximum starts at 0 as the device's does, and
    `NaN drives the max`: a NaN's bit pattern wins the device's integer atomic maximum, and a NaN maximum fails `> 0`, which gives 0.)"""
    v = np.asarray(W, np.float32).ravel()
    if not skip_nan and np.isnan(v).any():
        return 0
    v = v[~np.isnan(v)]
    m = np.float32(max(float((np.abs(v) if use_abs else v).max()), 0.0)) if v.size else np.float32(0.0)
    return floor_log2_f32(np.float32(448.0) / m) if m > 0 else 0


def w_exponents(ws):
    """fp8 weight exponents floor_log2(448 / max|W|), in float32."""
    return [w_exponent(ws[l]) for l in range(3)]


def act_exponents(rec, ws):
    """Calibrated activation exponents floor_log2(448 / (2 max|act_l|)) over the fp32 chain's exact activations, in float32."""
    acts, _ = fp32_acts(rec, ws)
    return [floor_log2_f32(np.float32(448.0) / (np.float32(2.0) * np.float32(np.abs(a).max()))) for a in acts]


def expected(prec, rec, ws, act_exp=None, w_exp=None):
    """The exact scores float32 [B] of the chain in precision `prec`."""
    fc = [ws[0].shape[0], ws[0].shape[1], ws[1].shape[1], ws[2].shape[1], 1]
    flat = [w.ravel() for w in ws]
    if prec == "f32":
        return fp32_acts(rec, ws)[1]
    if prec == "bf16":
        return chain_bf16_reference(np.asarray(rec, np.float32), flat, fc).ravel()
    return chain_fp8_reference(np.asarray(rec, np.float32), flat, fc, act_exp, w_exp).ravel()


def _lowbit(x):
    """min over the nonzero finite values of log2 of their lowest set bit (x = odd * 2^lowbit)."""
    a = np.abs(np.asarray(x, np.float64))
    a = a[(a > 0) & np.isfinite(a)]
    if a.size == 0:
        return None
    m, e = np.frexp(a)
    M = (m * 2.0 ** 53).astype(np.int64)
    tz = np.log2((M & -M).astype(np.float64)).astype(np.int64)
    return int((e - 53 + tz).min())


def operands(prec, rec, ws, act_exp=None, w_exp=None):
    """Per layer (FC1, FC2, FC3, output), the operands (A [B][K], W [K][N]) in the domain where the device multiplies and sums, and per
    hidden layer (value before, value after) the chain's rounding, in the next layer's operand domain: -> (ops, hidden)."""
    ops, hidden = [], []
    if prec == "fp8":
        dec = e4m3_decode_table()
        x = dec[e4m3_encode(np.asarray(rec, np.float32) * np.float32(2.0 ** act_exp[0]))]
        for l in range(3):
            Wf = dec[e4m3_encode(ws[l] * np.float32(2.0 ** w_exp[l]))]
            ops.append((x, Wf))
            r = ((x @ Wf) * 2.0 ** -(act_exp[l] + w_exp[l])).astype(np.float32) * np.float32(2.0 ** act_exp[l + 1])
            x = dec[e4m3_encode(r)]
            hidden.append((r.astype(np.float64), x))
        ops.append((x * 2.0 ** -act_exp[3], ws[3].astype(np.float64)))
        return ops, hidden
    rnd = (lambda v: v) if prec == "f32" else bf16_round
    x = rnd(np.asarray(rec, np.float32)).astype(np.float64)
    for l in range(3):
        W = rnd(ws[l]).astype(np.float64)
        ops.append((x, W))
        r = (x @ W).astype(np.float32)
        x = rnd(r).astype(np.float64)
        hidden.append((r.astype(np.float64), x))
    ops.append((x, rnd(ws[3]).astype(np.float64)))   # (the bf16 chain reads the bf16 vector of Wout, as chain_bf16_reference does)
    return ops, hidden


def premise(prec, rec, ws, act_exp=None, w_exp=None):
    """Assert the exactness premise: per layer, every product is a multiple of q = 2^(lowbit(A) + lowbit(W)) and every output's sum
    of |products| stays below 2^24 q, so every fp32 summation order is exact.  Items with a non-finite feature are left out.
    -> per layer (log2 q, max sum / (2^24 q))."""
    out = []
    rec = np.asarray(rec, np.float32)
    live = np.isfinite(rec).all(axis=1)
    ops, _ = operands(prec, rec[live], ws, act_exp, w_exp)
    for l, (A, W) in enumerate(ops):
        la, lw = _lowbit(A), _lowbit(W)
        if la is None or lw is None:
            out.append((None, 0.0))
            continue
        q = 2.0 ** (la + lw)
        worst = float((np.abs(A) @ np.abs(W)).max())
        assert worst < 2.0 ** 24 * q, "layer %d (%s): sum of |products| %g >= 2^24 * 2^%d" % (l, prec, worst, la + lw)
        out.append((la + lw, worst / (2.0 ** 24 * q)))
    return out


def rounding_witnesses(prec, rec, ws, act_exp=None, w_exp=None):
    """Per hidden layer: (values the chain's type must round, exact ties among them).  A tie lies half-way between two neighbours of the
    type, so round-to-nearest-even and round-half-away part on it."""
    _, hidden = operands(prec, rec, ws, act_exp, w_exp)
    res = []
    for r, x in hidden:
        inexact = r != x
        if prec == "bf16":
            u = np.ascontiguousarray(r, np.float32).view(np.uint32)
            tie = (u & 0xFFFF) == 0x8000
        elif prec == "fp8":
            a = np.abs(r)
            _, ex = np.frexp(a)
            q = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
            tie = (a <= 448.0) & (np.mod(a, q) == q / 2)
        else:
            tie = np.zeros(r.shape, bool)
        res.append((int(inexact.sum()), int(tie.sum())))
    return res


# ---- weights that must round: the master-weight side of the chain (pack kernels, fp8 weight exponents, the form of Wout) ------------------
# The stock weights {-2 .. 2} are exact in bf16 and in e4m3 at any power-of-two scale, so no pack kernel ever rounds them.  wide_weights()
# replaces every nonzero weight by a float32 value that the device's conversion must round:
#   bf16: a value of the closed interval that rounds (RNE) to w * 2^8 -- [255.5, 257] for |w| = 1, [511, 514] for |w| = 2.  Both ends are
#         exact ties that resolve to the even neighbour, the lower ends carry into the next binade.  The rounded image is the stock
#         image times 2^8, so every lowbit and every sum of premise() shifts by the same amount: the premise is inherited.
#   fp8:  a value of FP8_POOL (units in which the layer's maximum is 28, i.e. 448 at scale 2^4): e4m3 keeps four significant bits, so
#         the images 16 .. 28 are richer than the stock ones and premise() is asserted on them, not inherited.
# Each value is then scaled by the layer's 2^s (exact in float32).
def _in(v, toward):
    return float(np.nextafter(np.float32(v), np.float32(toward)))


BF16_PREIMAGES = {   # |stock| -> tie (carries), just inside it, above half, the exact value, below half, just inside the upper tie, upper tie
    1: (255.5, _in(255.5, 256), 255.75, 256.0, 256.5, _in(257, 256), 257.0),
    2: (511.0, _in(511, 512), 511.5, 512.0, 513.0, _in(514, 512), 514.0),
}
FP8_POOL = (17.0, 19.0, 21.0, 23.0, 25.0, 27.0,     # ties between the e4m3 neighbours 16, 18 .. 28: three resolve downward, three upward
            15.5,                                    # a tie that carries to 16
            19.01, 20.99, 23.5, 27.5, 16.99,         # near-ties, above and below half
            16.0, 24.0, 28.0,                        # exact
            2.0 ** -14)                              # half the smallest e4m3 subnormal at this scale: a tie that flushes to zero
FP8_TOPS = {28.0: 1.0, 27.0: 1.0, 3.5: 0.125}        # a layer's maximum at unit scale -> its unit: 28 * 2^4 = 448 exactly (the top of the interval
#                                                      (224, 448]), 27 * 2^4 = 432 (a tie, rounds to 448), 448 / 3.5 = 2^7 exactly (a power-of-two quotient)


def wide_weights(W, prec, s, seed, top=28.0):
    """The stock matrix W with every nonzero replaced (sign kept) by a value its image must round, times 2^s; every value of the
    pool is used, the layer's maximum is `top` * 2^s in fp8 (514 * 2^s in bf16)."""
    rng = np.random.default_rng(seed)
    W = np.ascontiguousarray(W, np.float32)
    out = np.zeros(W.size, np.float32)
    flat = W.ravel()
    if prec == "bf16":
        for a, vals in BF16_PREIMAGES.items():
            sel = np.flatnonzero(np.abs(flat) == a)
            pool = np.array(vals, np.float32)
            assert sel.size >= pool.size
            out[sel] = np.sign(flat[sel]) * pool[rng.permutation(sel.size) % pool.size]
        assert np.count_nonzero(out) == np.count_nonzero(flat)
    else:
        unit = FP8_TOPS[top]
        pool = np.array([v for v in FP8_POOL if v * unit <= top], np.float32) * np.float32(unit)
        sel = np.flatnonzero(flat)
        assert sel.size >= pool.size
        out[sel] = np.sign(flat[sel]) * pool[rng.permutation(sel.size) % pool.size]
        assert np.abs(out).max() == np.float32(top)
    return (out * np.float32(2.0 ** s)).reshape(W.shape)


def wide_wout(W, s=0):
    """The fp8 chain's output layer reads the fp32 master: t * 257 / 256 needs nine significant bits, so a bf16 image of it differs."""
    return (np.ascontiguousarray(W, np.float32) * np.float32(257.0 / 256.0) * np.float32(2.0 ** s)).astype(np.float32)


def bf16_image(W, mode="rne"):
    """float32 -> bf16 as float32: round to nearest even (the device), or the mutants `trunc` (toward zero) and `away` (half away)."""
    if mode == "rne":
        return bf16_round(W)
    u = np.ascontiguousarray(W, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + (0x8000 if mode == "away" else 0)) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(np.shape(W))


def e4m3_image(v, mode="rne"):
    """The e4m3 value (float64) of float32 v: clamp to +-448, then round to nearest even (== the decode of gpu_helpers.e4m3_encode), or
    the mutants `trunc` and `away`."""
    x = np.clip(np.asarray(v, np.float32), -448.0, 448.0).astype(np.float64)
    a = np.abs(x)
    _, ex = np.frexp(a)
    q = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
    t = a / q
    t = np.rint(t) if mode == "rne" else np.floor(t) if mode == "trunc" else np.floor(t + 0.5)
    return np.copysign(t * q, x)


def weight_image(prec, l, W, w_exp=None, mode="rne"):
    """What the kernels of precision `prec` multiply by for layer l (float64, in the domain they sum in): the fp32 master (the fp32 chain, and
    the fp8 chain's output layer), its bf16 image, or the e4m3 image of W * 2^w_exp[l]."""
    if prec == "f32" or (prec == "fp8" and l == 3):
        return np.asarray(W, np.float64)
    if prec == "bf16":
        return bf16_image(W, mode).astype(np.float64)
    return e4m3_image(np.asarray(W, np.float32) * np.float32(2.0 ** w_exp[l]), mode)


def weight_witnesses(prec, l, W, w_exp=None):
    """Of one layer's weights: (values the image must round, exact ties resolved toward zero, ties resolved away from zero, roundings that carry
    into the next binade)."""
    v = np.asarray(W, np.float32)
    if prec == "fp8":
        v = v * np.float32(2.0 ** w_exp[l])
    img = weight_image(prec, l, W, w_exp)
    a, b = np.abs(v.astype(np.float64)), np.abs(img)
    if prec == "bf16":
        tie = (np.ascontiguousarray(v).view(np.uint32) & 0xFFFF) == 0x8000
    else:
        _, ex = np.frexp(a)
        q = np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)
        tie = (a <= 448.0) & (np.mod(a, q) == q / 2)
    carry = (b > a) & (np.frexp(b)[1] > np.frexp(a)[1])
    return int((a != b).sum()), int((tie & (b < a)).sum()), int((tie & (b > a)).sum()), int(carry.sum())


def exponent_margin(quotients):
    """min over float64 quotients q of |q / 2^round(log2 q) - 1|: how far the nearest one lies from a power of two, where its floor_log2 would
    flip.  The device finds a maximum or a sum of squares in fp32 and in no fixed order; a margin far above 2^-20 makes its exponent certain."""
    q = np.asarray(quotients, np.float64)
    return float(np.abs(q / np.exp2(np.rint(np.log2(q))) - 1.0).min())


def act_exponent_quotients(rec, ws):
    acts, _ = fp32_acts(rec, ws)
    return [448.0 / (2.0 * float(np.abs(a).max())) for a in acts]


def estimated_act_exponents(ws, fc):
    """The activation exponents of an uncalibrated fp8 context (fr_api.cpp f8_estimate_act_exponents): rms 0.58 at the input, times
    sqrt(sum W_l^2 / H_l) per layer, 8 rms must fit 448.  -> (exponents, the float64 quotients they are the floor_log2 of)."""
    rms, out, quot = 0.58, [], []
    for l in range(4):
        quot.append(448.0 / (8.0 * rms))
        out.append(floor_log2_f32(np.float32(448.0) / (np.float32(8.0) * np.float32(rms))))
        if l < 3:
            rms *= float(np.sqrt((ws[l].astype(np.float64) ** 2).sum() / fc[l + 1]))
    return out, quot


# ---- the GPU matrix: (model, precision, batch, chain width, stream group) -> the kernels fr_worker_last_kernel must report ----------------
# MODELS: name -> (K, hidden widths, dense_len).  A case's `stream` is the kernel of the streamed launch (push_device with `group` batches
# queued; None = the stage pipeline, which no hook names), `layers` what fc_layer_only(batch, l) reports for l = 0..3 (None: not asserted),
# `runs` the stage-pipeline kernels its submits and pushes launch that no hook reports, `gather_out` (one of them) what the fifth of five pushes
# in flight launches: the gather of the fifth batch and the output layer of the first in one launch, every FC layer between them a GEMM launch
# (fr_api.cpp pipeline_step, fr_pipeline.hip pipeline_launch_prec; a push on the stage pipeline leaves fr_worker_last_kernel untouched).
MODELS = {
    "A352": (352, (1024, 512, 256), 0),
    "B880": (880, (1024, 512, 256), 16),
    "F512": (512, (1024, 512, 256), 0),
    "F256": (256, (1024, 512, 256), 0),
    "G512": (512, (1024, 256, 256), 0),
    "G256": (256, (1024, 256, 256), 0),
    "H528": (528, (1024, 512, 256), 0),
    "H704": (704, (1024, 512, 256), 16),
    "C": (3968, (2048, 512, 256), 16),
    "Q": (3968, (2048, 768, 256), 16),
    "P": (4200, (2048, 512, 256), 8),
    "K128": (128, (2048, 512, 256), 0),
    "K256": (256, (2048, 512, 256), 0),
    "N192": (512, (192, 256, 256), 0),
    "R": (3968, (2048, 512, 512), 16),
}


def model_spec(name):
    K, fc, dl = MODELS[name]
    return spec(K, fc, dense_len=dl, name="exact_" + name)


def model_seed(name):
    return 7000 + sum(ord(c) for c in name)


PIPE = "fr_pipeline_kernel<%d, %d>"


def _pipe_layers(p):
    return [PIPE % (s, p) for s in (1, 2, 3, 4)]


CASES = [
    # fp32 fused item-tile kernels (a push group below 12 batches rides the stage pipeline); the stage pipeline per layer
    dict(id="f32-A352-g16", model="A352", prec="f32", batch=256, group=16, stream="fr_fused_tile_kernel<2, 44, 4, false>", layers=_pipe_layers(0)),
    dict(id="f32-A352-g64", model="A352", prec="f32", batch=256, group=64, stream="fr_fused_tile_m2_kernel<44>"),
    dict(id="f32-B880", model="B880", prec="f32", batch=200, group=16, stream="fr_fused_tile_kernel<2, 110, 2, false>"),
    dict(id="f32-F512", model="F512", prec="f32", batch=128, group=16, stream="fr_fused_tile_kernel<2, 0, 2, true>"),
    dict(id="f32-F256", model="F256", prec="f32", batch=128, group=16, stream="fr_fused_tile_kernel<2, 0, 2, false>"),
    dict(id="f32-G512", model="G512", prec="f32", batch=128, group=16, stream="fr_fused_tile_kernel<1, 0, 2, true>"),
    dict(id="f32-G256", model="G256", prec="f32", batch=128, group=16, stream="fr_fused_tile_kernel<1, 0, 2, false>"),
    # bf16 / fp8 fused kernels: chunked (small launches), persistent (from about one tile per CU on; any launch for other records), fp8
    dict(id="bf16-A352-g16", model="A352", prec="bf16", batch=256, group=16, stream="fr_fused_tile_h_kernel<2, 2, 22, true, 16, 2>", layers=_pipe_layers(1)),
    dict(id="bf16-B880-g16", model="B880", prec="bf16", batch=256, group=16, stream="fr_fused_tile_h_kernel<2, 2, 55, false, 12, 2>"),
    dict(id="bf16-A352-g64", model="A352", prec="bf16", batch=256, group=64, stream="fr_fused_tile_hs_kernel<1, 22, 4, 16, 3, 4, 0, 0, 0>"),
    dict(id="bf16-H528", model="H528", prec="bf16", batch=200, group=16, stream="fr_fused_tile_hs_kernel<1, 33, 6, 32, 3, 4, 0, 0, 0>"),
    dict(id="bf16-H704", model="H704", prec="bf16", batch=200, group=16, stream="fr_fused_tile_hs_kernel<1, 44, 6, 32, 2, 6, 0, 0, 0>"),
    dict(id="bf16-B880-g128", model="B880", prec="bf16", batch=256, group=128, stream="fr_fused_tile_hs_kernel<1, 55, 7, 32, 2, 6, 0, 0, 0>"),
    dict(id="fp8-A352", model="A352", prec="fp8", batch=256, group=16, stream="fr_fused_tile_f8_kernel<6>", layers=_pipe_layers(2)),
    dict(id="fp8-B880", model="B880", prec="fp8", batch=100, group=16, stream="fr_fused_tile_f8_kernel<14>"),
    # the stage pipeline at Model-C shapes (fp32 split-K at few tiles), ragged batches below any GEMM ldm.  Every submit starts with a
    # gather-only step; four pushes before sync() keep several batches in flight, so their steps launch the multi-stage kernel
    *[dict(id="%s-C-b%d" % (p, b), model="C", prec=p, batch=b, group=1 if b < 33 else 4, stream=None, layers=_pipe_layers(i) if b == 65 else None,
           runs=[PIPE % (0, i)] + ([PIPE % (-1, i)] if b >= 33 else []))
      for i, p in enumerate(PRECS) for b in ((1, 31, 33, 65, 200) if p == "f32" else (33, 65))],
    # GEMM tiles on the full chip (W = 1) at batch 4096: 128 x 256 FC1, 64 x 128 FC2, FC3 + output layer in one launch (bf16 / fp8)
    dict(id="f32-C-4096", model="C", prec="f32", batch=4096, width=1, group=1, stream=None, gather_out="fr_gather_out_kernel<0>",
         layers=["fc_lp_gemm_kernel<0, 2, 128, 2, 8, 32>", "fc_lp_gemm_kernel<0, 1, 64, 2, 8, 32>", "fc_lp_gemm_kernel<0, 1, 64, 2, 8, 32>", PIPE % (4, 0)]),
    dict(id="bf16-C-4096", model="C", prec="bf16", batch=4096, width=1, group=1, stream=None,
         layers=["fc_pp_gemm_n128_kernel<1, 2>", "fc_lp_gemm_kernel<1, 1, 64, 4, 8, 32>", "fc_lp_gemm_out_kernel<1, 2>", PIPE % (4, 1)]),
    dict(id="fp8-C-4096", model="C", prec="fp8", batch=4096, width=1, group=1, stream=None,
         layers=["fc_pp_gemm_n128_kernel<2, 2>", "fc_lp_gemm_kernel<2, 1, 64, 2, 8, 32>", "fc_lp_gemm_out_kernel<2, 2>", PIPE % (4, 2)]),
    # FC3 with 512 outputs: a GEMM launch (64 x 128 tiles), but no fused FC3 + output tail (that one takes 256 outputs) -- the output layer stays a
    # stage of the pipeline, so five batches in flight launch fr_gather_out_kernel in bf16 and fp8 too
    *[dict(id="%s-R-4096" % p, model="R", prec=p, batch=4096, width=1, group=1, stream=None, gather_out="fr_gather_out_kernel<%d>" % i,
           layers=[None, None, None, PIPE % (4, i)]) for i, p in ((1, "bf16"), (2, "fp8"))],
    # 128 x 128 tiles: ldm 1664 = 13 * 128 (26 pad items)
    *[dict(id="%s-C-1638" % p, model="C", prec=p, batch=1638, width=1, group=1, stream=None,
           layers=["fc_lp_gemm_kernel<%d, 1, 128, 2, 8, 32>" % i, PIPE % (2, i), PIPE % (3, i), PIPE % (4, i)]) for i, p in enumerate(PRECS)],
    # 256 x 256 tiles (chain width 4): N = 2048 / 512 / 768
    dict(id="bf16-C-4096-w4", model="C", prec="bf16", batch=4096, width=4, group=1, stream=None,
         layers=["fc_pp_gemm_kernel<1, 3, 8>", "fc_pp_gemm_kernel<1, 3, 2>", "fc_lp_gemm_out_kernel<1, 2>", None]),
    dict(id="fp8-C-4096-w4", model="C", prec="fp8", batch=4096, width=4, group=1, stream=None,
         layers=["fc_pp_gemm_kernel<2, 2, 8>", "fc_pp_gemm_kernel<2, 2, 2>", "fc_lp_gemm_out_kernel<2, 2>", None]),
    dict(id="bf16-Q-4096-w4", model="Q", prec="bf16", batch=4096, width=4, group=1, stream=None, layers=[None, "fc_pp_gemm_kernel<1, 3, 0>", None, None]),
    dict(id="fp8-Q-4096-w4", model="Q", prec="fp8", batch=4096, width=4, group=1, stream=None, layers=[None, "fc_pp_gemm_kernel<2, 2, 0>", None, None]),
    # N = 192 (an odd multiple of 64) at ldm 5504 = 43 * 128: 64 x 128 tiles
    *[dict(id="%s-N192-5500" % p, model="N192", prec=p, batch=5500, width=1, group=1, stream=None,
           layers=["fc_lp_gemm_kernel<%d, 1, 64, %d, 8, 32>" % (i, 4 if i == 1 else 2), None, None, None]) for i, p in enumerate(PRECS)],
    # KE / 8 == 2: 128 x 256 tiles on fc_lp_gemm_kernel (too few k-steps for the phased-waves kernel)
    dict(id="bf16-K128-4096", model="K128", prec="bf16", batch=4096, width=1, group=1, stream=None, layers=["fc_lp_gemm_kernel<1, 2, 128, 2, 8, 32>", None, None, None]),
    dict(id="fp8-K256-4096", model="K256", prec="fp8", batch=4096, width=1, group=1, stream=None, layers=["fc_lp_gemm_kernel<2, 2, 128, 2, 8, 32>", None, None, None]),
    # fp8 with K % 64 != 0 (zero-padded to 66 * 64 k inside the operand image; the bf16 chain refuses a K that is not a multiple of 16)
    dict(id="fp8-P-4096", model="P", prec="fp8", batch=4096, width=1, group=1, stream=None, layers=["fc_pp_gemm_n128_kernel<2, 2>", None, None, None]),
]

# Kernels of libfleetrec.so that no shape, batch, chain width or stream group reaches (the product reads no environment variables).
UNREACHABLE = {}


# ---- the shape sweep: every FC-chain kernel at the edges of the ranges its dispatch predicate accepts -------------------------------------
# A row is a case with its own shape: spec (K, (H1, H2, H3), dense_len), prec, batch, width, group; `edge` says which edge it sits on,
# `layer` which of FC1 / FC2 / FC3 / stream is swept and `kernel` what fr_worker_last_kernel reports for it (fc_layer_only of that layer, or the
# streamed launch of `group` pushes).  `family` / `cover` feed the coverage table; the remaining keys say where the edge bites, for the
# mutants of tests/test_exact_chain_cpu.py: `kstep` = k per K step of the swept layer's loop, `pad` = (k per k-group, K padded) where the
# kernel zero-pads the swept layer's K, `chunks` = H1 / 256 where the kernel loops over H1 chunks, `split` = the stage pipeline's split-K plan.
LP, PPN, PP, OUT = "fc_lp_gemm_kernel<%d, %d, %d, %d, 8, 32>", "fc_pp_gemm_n128_kernel<%d, 2>", "fc_pp_gemm_kernel<%d, %d, %d>", "fc_lp_gemm_out_kernel<%d, 2>"
FUSED, HS = "fr_fused_tile_kernel<%d, 0, 2, %s>", "fr_fused_tile_hs_kernel<1, %s, 0, 0, 0>"
_PI = {"f32": 0, "bf16": 1, "fp8": 2}
_KROW = {"f32": 4, "bf16": 8, "fp8": 16}   # k per element row of the GEMM operand images
C_FC = (2048, 512, 256)


def pick_nsplit(K, N, ldm):
    """The stage pipeline's split-K plan of one fp32 layer (fr_api.cpp pick_nsplit)."""
    return 2 if ((N // 32) * (ldm // 32) < 256 and (K // 8) % 16 == 0 and (K // 8) // 16 >= 4) else 1


def split_plan(row):
    """(FC1, FC2, FC3) split counts of a row's stage-pipeline run: fp32 only, the low-precision chains never split."""
    K, fc, _ = row["spec"]
    ldm = (row["batch"] + 31) // 32 * 32
    dims = [K] + list(fc)
    return tuple(pick_nsplit(dims[l], dims[l + 1], ldm) if row["prec"] == "f32" else 1 for l in range(3))


def gemm_steps(prec, K):
    """K steps of 8 element rows the GEMM kernels take for a layer of K inputs (fp8 pads K to a multiple of 64)."""
    return ((K + 63) // 64 * 4 if prec == "fp8" else K // _KROW[prec]) // 8


def fused_db(K, H2):
    """Which fr_fused_tile_kernel<.., 0, 2, DB> the LDS arithmetic of frk_fused_launch picks (fr_fused.hip: rows of 33 16-byte elements)."""
    single = max(K // 4 + 64, max(H2 // 4, 68)) * 33 * 16
    double = max(K // 4 + 128, H2 // 4 + 68) * 33 * 16
    assert single <= 160 * 1024, (K, H2)
    return single > 80 * 1024 and double <= 160 * 1024


def _hs_kernel(K):
    return HS % ("22, 4, 16, 3, 4" if K <= 352 else "33, 6, 32, 3, 4" if K <= 528 else "44, 6, 32, 2, 6" if K <= 704 else "55, 7, 32, 2, 6")


def _row(family, prec, K, fc, batch, layer, kernel, edge, cover, width=1, group=1, dense_len=0, tag="", **where):
    rid = "%s-%s-K%d-%s-b%d%s" % (family, prec, K, "x".join(map(str, fc)), batch, tag)
    return dict(id=rid, family=family, spec=(K, tuple(fc), dense_len), prec=prec, batch=batch, width=width, group=group, layer=layer, kernel=kernel,
                edge=edge, cover=cover, **where)


def _gemm_row(family, prec, K, fc, layer, kernel, edge, batch=4090, **kw):
    """A GEMM-tile row: the swept layer's K is record K (FC1), H1 (FC2) or H2 (FC3)."""
    KL = {"FC1": K, "FC2": fc[0], "FC3": fc[1]}[layer]
    steps = gemm_steps(prec, KL)
    pad = {"pad": (16, (KL + 63) // 64 * 64)} if prec == "fp8" and KL % 64 else {}
    cover = "nsub=%d" % (2 * steps) if family == "t256" else "steps=%d" % steps
    return _row(family, prec, K, fc, batch, layer, kernel, "%s (%d K steps)" % (edge, steps), cover, kstep=8 * _KROW[prec], **pad, **kw)


def _sweeps():
    rows = []
    # 128 x 256 tiles, FC1 of (2048, 512, 256) on the whole chip: 2 K steps ride the plain loop, 3 (nsub == D + 1), 4, 5 the phased-waves kernel
    for prec, Ks in (("bf16", (128, 192, 256, 320)), ("fp8", (256, 384, 512, 640, 328)), ("f32", (64, 96, 128, 160))):
        for K in Ks:
            st, p = gemm_steps(prec, K), _PI[prec]
            pp = prec != "f32" and st >= 3
            rows.append(_gemm_row("n128", prec, K, C_FC, "FC1", PPN % p if pp else LP % (p, 2, 128, 2),
                                  ("phased waves, nsub == D + 1: one memory phase issues a DMA" if pp and st == 3 else
                                   "phased waves, nsub == D + %d" % (st - 2) if pp else "plain two-stage loop") +
                                  (", K zero-padded to 384" if K == 328 else "")))
    # 256 x 256 tiles (chain width 4): sub-steps of 4 element rows, bf16 D = 3, fp8 D = 2; N = 2048 (XCD tile map) and N = 768 (linear map)
    for K in (128, 192, 256):
        for fc, nt in ((C_FC, 8), ((768, 512, 256), 0)):
            nsub = K // 8 // 4
            rows.append(_gemm_row("t256", "bf16", K, fc, "FC1", PP % (1, 3, nt), "256 x 256 phased waves, nsub == %d == D + %d" % (nsub, nsub - 3), width=4))
    for K in (256, 384):   # KE % 8 == 0 makes nsub even: nsub == D + 1 == 3 cannot be reached in fp8
        nsub = K // 16 // 4
        rows.append(_gemm_row("t256", "fp8", K, C_FC, "FC1", PP % (2, 2, 8), "256 x 256 phased waves, nsub == %d == D + %d" % (nsub, nsub - 2), width=4))
    # 64 x 128 tiles, FC2 (K = H1, N = 512): bf16 rides a ring of S = 4 stages -- 2, 3 steps (fewer than the ring), 4, 5 (not a multiple of it)
    for prec, H1s in (("bf16", (128, 192, 256, 320)), ("fp8", (256, 384)), ("f32", (64, 96))):
        for H1 in H1s:
            S = 4 if prec == "bf16" else 2
            rows.append(_gemm_row("t64", prec, 512, (H1, 512, 256), "FC2", LP % (_PI[prec], 1, 64, S), "64 x 128 tiles, ring of %d" % S))
    # 128 x 128 tiles: ldm 1664 = 13 * 128, three K steps on the ring of two
    for prec, K in (("f32", 96), ("bf16", 192), ("fp8", 384)):
        rows.append(_gemm_row("t128", prec, K, C_FC, "FC1", LP % (_PI[prec], 1, 128, 2), "128 x 128 tiles, ring of 2", batch=1638))
    # FC3 + the output layer in one launch (K = H2, N = 256): its accepted minimum of two K steps, and three
    for prec, H2s in (("bf16", (128, 192)), ("fp8", (256, 384))):
        for H2 in H2s:
            rows.append(_gemm_row("tail", prec, 512, (512, H2, 256), "FC3", OUT % _PI[prec], "FC3 + output tail, ring of 2"))
    # fp32 fused kernel, generic-K form: K in blocks of four k-groups of 8; the LDS layout (and DB) follows K and H2
    for H2, Ks in ((512, (32, 96, 384, 704, 736, 960)), (256, (32, 960))):
        for K in Ks:
            db = fused_db(K, H2)
            single = max(K // 4 + 64, max(H2 // 4, 68)) * 33 * 16 <= 80 * 1024
            edge = "generic K, %d blocks of 32 k, %s" % (K // 32, "single-buffer layout (two workgroups per CU)" if single else
                                                         "double-buffered R1" if db else "one workgroup per CU, single R1 buffer (wpe == 2 && !db)")
            for batch in (33, 200):
                rows.append(_row("fused32", "f32", K, (512, H2, 256), batch, "stream", FUSED % (2 if H2 == 512 else 1, "true" if db else "false"), edge,
                                 "K=%d/H2=%d" % (K, H2), group=16, dense_len=16 if K == 960 else 0, kstep=32,
                                 **({"rows": 400} if K == 32 else {})))   # (a record of one table: enough rows for distinct items)
    # H1 chunk counts 1 and 3 in every fused kernel with a chunk loop (H1 = 1024, four chunks, is the GPU matrix's)
    for H1 in (256, 768):
        edge = "%d H1 chunk%s of 256%s" % (H1 // 256, "" if H1 == 256 else "s", ": the double buffer never alternates" if H1 == 256 else ": an odd count")
        fc = (H1, 512, 256)
        for prec, K, batch, group, kern in (("f32", 352, 100, 16, "fr_fused_tile_kernel<2, 44, 4, false>"), ("f32", 512, 100, 16, FUSED % (2, "true")),
                                            ("f32", 352, 256, 64, "fr_fused_tile_m2_kernel<44>"),
                                            ("bf16", 352, 100, 16, "fr_fused_tile_h_kernel<2, 2, 22, true, 16, 2>"),
                                            ("bf16", 880, 100, 16, "fr_fused_tile_h_kernel<2, 2, 55, false, 12, 2>"),
                                            ("fp8", 352, 100, 16, "fr_fused_tile_f8_kernel<6>"), ("fp8", 880, 100, 16, "fr_fused_tile_f8_kernel<14>")):
            rows.append(_row("chunks", prec, K, fc, batch, "stream", kern, edge, "chunks=%d" % (H1 // 256), group=group, dense_len=16 if K == 880 else 0,
                             chunks=H1 // 256))
    # the persistent bf16 kernel below the top of each instantiation: zero k-groups past the record, partial slices
    for K in (64, 80, 368, 544, 720, 864):
        top = 352 if K <= 352 else 528 if K <= 528 else 704 if K <= 704 else 880
        for batch in (65, 200):
            rows.append(_row("hs", "bf16", K, (1024, 512, 256), batch, "stream", _hs_kernel(K), "%d k-groups of 16 in an instantiation of %d: %d zero k-groups" % (
                K // 16, top // 16, (top - K) // 16), "kgroups=%d/%d" % (K // 16, top // 16), group=16, dense_len=16 if K == 720 else 0, kstep=16, pad=(16, top),
                **({"table_max": 12} if K <= 80 else {})))
    # the stage pipeline: split-K plans, the fp8 gather of a record with K % 64 != 0, a bf16 record with K % 32 == 16
    for K, fc, layers in ((640, (384, 512, 256), ("FC2", "FC3")), (576, (640, 384, 256), ("FC2", "FC3")), (384, (512, 256, 256), ("FC1", "FC2")),
                          (576, (384, 384, 256), ("FC2", "FC3"))):
        for batch, layer in zip((33, 200), layers):
            r = _row("stage", "f32", K, fc, batch, layer, None, "", "")
            ns = split_plan(r)
            s = int(layer[2])
            reads, own = (1 if s == 1 else ns[s - 2]), ns[s - 1]
            r.update(kernel=PIPE % (s, 0), split=ns, cover="split=%d%d%d" % ns,
                     edge="split-K plan %s: %s reads %d partial%s and writes %d" % (ns, layer, reads, "" if reads == 1 else "s", own))
            rows.append(r)
    for K, fc, dl in ((104, (256, 512, 256), 0), (4200, C_FC, 8)):   # (104: a model's record is a multiple of 8 floats, so K = 100 cannot be built)
        rows.append(_row("stage", "fp8", K, fc, 33, "FC1", PIPE % (1, 2), "the stage pipeline's own q16 gather, K %% 64 == %d (zero-padded to %d)" % (K % 64, (K + 63) // 64 * 64),
                         "K%%64=%d" % (K % 64), dense_len=dl, kstep=64, pad=(16, (K + 63) // 64 * 64)))
    for K in (48, 112):
        rows.append(_row("stage", "bf16", K, (256, 512, 256), 33, "FC1", PIPE % (1, 1), "bf16 record with K % 32 == 16: an odd count of k-groups of 16",
                         "K%32=16", kstep=16, pad=(16, (K + 31) // 32 * 32), **({"table_max": 12} if K == 48 else {})))
    return rows


SWEEPS = _sweeps()

# Per kernel family: the range its dispatch predicate accepts, and what the sweep leaves out on purpose (the coverage table).
FAMILIES = {
    "n128": ("lp_gemm_mu == 2 (N % 128 == 0, ldm % 256 == 0, N / 128 * ldm / 256 >= 192): K steps = KE / 8 >= 2; 2 -> fc_lp_gemm_kernel<P, 2, 128, 2>, "
             ">= 3 -> fc_pp_gemm_n128_kernel<P, 2> (bf16 / fp8), every count -> fc_lp_gemm_kernel<0, 2, 128, 2> (f32)",
             "steps above 5 are the steady state the GPU matrix runs (K = 3968, 4200); other N / ldm change the grid only"),
    "t256": ("lp_gemm_mu == 6 (bf16 / fp8, N % 256 == 0, ldm % 256 == 0, N / 256 * ldm / 256 >= 192 / width): nsub = KE / 4 >= 4, even",
             "fp8 nsub == D + 1 == 3: KE % 8 == 0 makes nsub even, the predicate cannot produce it; NT = 2 (N = 512) needs FC2's K = H1 = 2048 "
             "for its tile count, so it stays at the GPU matrix's one shape"),
    "t64": ("lp_gemm_mu == 3 (N % 64 == 0, ldm % 128 == 0, N / 64 * ldm / 128 >= 128, larger tiles short of the chip): K steps >= 2, ring of 4 (bf16) / 2",
            "steps above 5: the GPU matrix (K = 2048); fp8 / f32 ring of 2 has no fewer-than-ring case besides 2 and 3 steps, both run"),
    "t128": ("lp_gemm_mu == 1 (N % 128 == 0, ldm % 128 == 0, N / 128 * ldm / 128 >= 192 or >= 64 where 64 x 128 tiles fall short): K steps >= 2",
             "2 steps on this tile: the ring logic is the n128 family's fc_lp_gemm_kernel<P, 2, 128, 2> (same body, S = 2), run there at 2 steps"),
    "tail": ("frk_fc_tail_ok (bf16 / fp8, N == 256, ldm % 128 == 0, K steps >= 2) and lp_gemm_mu != 0",
             "f32 has no fused tail; steps above 3: the GPU matrix (H2 = 512, 768)"),
    "fused32": ("frk_fused_ok, generic K: K % 32 == 0 up to the LDS bound K = 960, H1 % 256 == 0, H2 in {256, 512}, H3 == 256",
                "K = 352 / 880 with H2 = 512 are the straight-line instantiations (GPU matrix, chunks family)"),
    "chunks": ("every fused kernel with a chunk loop: H1 % 256 == 0 (fr_fused_tile_kernel, _m2_kernel, _h_kernel, _f8_kernel)",
               "four chunks: the GPU matrix; two chunks: the fused32 family (H1 = 512); fr_fused_tile_hs_kernel takes H1 == 1024 only"),
    "hs": ("frk_fused_hk_ok: K % 16 == 0, 64 <= K <= 880, hidden (1024, 512, 256); the narrowest of 22 / 33 / 44 / 55 k-groups that holds K",
           "the top of each instantiation (K = 352 / 528 / 704 / 880): the GPU matrix"),
    "stage": ("pick_nsplit: 2 where K % 128 == 0, K >= 512 and fewer than 256 tiles of 32 x 32 (fp32 only); any record (K % 8 == 0) in fp8, K % 16 == 0 in bf16",
              "plans (2, 2, 2) and (1, 2, 2): the GPU matrix (Model C)"),
}


# ---- the weight rows: one per precision for each distinct reader of a weight image, on weights that must round -----------------------------
# A row runs like a sweep row, on the shape of the smallest CASES / SWEEPS entry that reaches its reader.  `wide`: the layers whose weights
# wide_weights() replaces (bf16: all four, Wout included; fp8: W1..W3, the images) -- or (3,) for the fp8 chain's fp32-master Wout, rows
# of their own (`wout`) on smaller-magnitude data: nine significant bits in Wout cost 257 x the headroom of premise()'s output layer.
# `layer`: FC1 / FC2 / FC3 / OUT = the layer whose fc_layer_only launch must report `kernel`, stream = the streamed launch of `group` pushes,
# stages = all four layers on the stage pipeline, gather_out = five pushes in flight (fr_gather_out_kernel<P>, which no hook reports).
BF16_SCALES = (-8, -7, -9, -8)                       # net factor 2^(8 + s) = 1, 2, 1/2, 1: the scores are the stock scores
FP8_LAYERS = ((28.0, 1), (27.0, -2), (3.5, 0))       # (top, s) per hidden layer -> w_exp 3, 6, 7
WOUT_SHRINK = dict(table_max=1, nnz=(12, 3, 2))   # tables in {-1, 0, 1}, 12 / 3 / 2 nonzeros per column of W1 / W2 / W3 (where K > N the cover of every row sets the floor)
R_FC = (2048, 512, 512)


def _wide_row(tag, prec, K, fc, batch, layer, kernel, reader, wout=False, width=1, group=1, dense_len=0):
    return dict(id="wide-%s-%s%s" % (prec, tag, "-wout" if wout else ""), spec=(K, tuple(fc), dense_len), prec=prec, batch=batch, width=width,
                group=group, layer=layer, kernel=kernel, reader=reader, wout=wout,
                wide=(3,) if wout else (0, 1, 2, 3) if prec == "bf16" else (0, 1, 2), **(WOUT_SHRINK if wout else {}))


def _wide_rows():
    A, C = (1024, 512, 256), C_FC
    rows = [
        _wide_row("fused_h", "bf16", 352, A, 256, "stream", "fr_fused_tile_h_kernel<2, 2, 22, true, 16, 2>", "chunked fused kernel: W1..W3 images, bf16 Wout", group=16),
        _wide_row("fused_hs", "bf16", 352, A, 256, "stream", _hs_kernel(352), "persistent fused kernel: buffer resources sized from the images", group=64),
        _wide_row("fused_f8", "fp8", 352, A, 256, "stream", "fr_fused_tile_f8_kernel<6>", "fp8 fused kernel: e4m3 images", group=16),
        _wide_row("fused_f8", "fp8", 352, A, 256, "stream", "fr_fused_tile_f8_kernel<6>", "fp8 fused kernel: fp32 Wout", group=16, wout=True),
    ]
    for prec in ("bf16", "fp8"):
        p = _PI[prec]
        k3, k2 = (192, 128) if prec == "bf16" else (384, 256)   # three / two K steps of the GEMM loops
        rows += [
            _wide_row("stages", prec, 3968, C, 65, "stages", None, "stage pipeline, stages 1-4", group=4, dense_len=16),
            _wide_row("n128", prec, k3, C, 4090, "FC1", PPN % p, "128 x 256 tiles, phased waves"),
            _wide_row("t256", prec, k2, C, 4090, "FC1", PP % (p, 3 if prec == "bf16" else 2, 8), "256 x 256 tiles (chain width 4)", width=4),
            _wide_row("t64", prec, 512, (k2, 512, 256), 4090, "FC2", LP % (p, 1, 64, 4 if prec == "bf16" else 2), "64 x 128 tiles"),
            _wide_row("t128", prec, k3, C, 1638, "FC1", LP % (p, 1, 128, 2), "128 x 128 tiles"),
            _wide_row("tail", prec, 512, (512, k2, 256), 4090, "FC3", OUT % p, "FC3 + output layer in one launch"),
            _wide_row("gather_out", prec, 3968, R_FC, 4096, "gather_out", "fr_gather_out_kernel<%d>" % p, "gather | output layer in one launch", dense_len=16),
        ]
    rows += [
        _wide_row("kpad", "fp8", 104, (256, 512, 256), 33, "FC1", PIPE % (1, 2), "K % 64 == 40: the zero K padding of the e4m3 image beside weights that round"),
        _wide_row("stages", "fp8", 3968, C, 65, "OUT", PIPE % (4, 2), "stage 4: fp32 Wout", wout=True, group=4, dense_len=16),
        _wide_row("tail", "fp8", 512, (512, 256, 256), 4090, "FC3", OUT % 2, "FC3 + output tail: fp32 Wout", wout=True),
        _wide_row("gather_out", "fp8", 3968, R_FC, 4096, "gather_out", "fr_gather_out_kernel<2>", "gather | output layer: fp32 Wout", wout=True, dense_len=16),
    ]
    return rows


WIDE = _wide_rows()


def widen(row, ws):
    """The row's weights: the stock ones with the layers of row['wide'] replaced (wide_weights / wide_wout), seeds derived from its id."""
    seed = zlib.crc32(row["id"].encode())
    out = list(ws)
    for l in row["wide"]:
        if row["prec"] == "bf16":
            out[l] = wide_weights(ws[l], "bf16", BF16_SCALES[l], seed + l)
        elif l == 3:
            out[l] = wide_wout(ws[l])
        else:
            out[l] = wide_weights(ws[l], "fp8", FP8_LAYERS[l][1], seed + l, top=FP8_LAYERS[l][0])
    return out


def named_kernels():
    """Every kernel name a GPU-matrix case asserts, or runs where no hook reports it (a case's `runs`: the stage pipeline's gather-only
    first step and its multi-stage steps, which fr_worker_last_kernel does not record)."""
    out = set()
    for c in CASES:
        out.update(c.get("runs") or [])
        if c.get("stream"):
            out.add(c["stream"])
        if c.get("gather_out"):
            out.add(c["gather_out"])
        out.update(n for n in (c.get("layers") or []) if n)
    return out


def case_data(case, n_items):
    """(spec, data, idx, dense) of a case or a sweep row: n_items rows drawn (with repetition) from its model's pool."""
    if "spec" in case:   # a SWEEPS row: its own shape, a seed derived from its id
        K, fc, dl = case["spec"]
        sp = spec(K, fc, dense_len=dl, rows=case.get("rows", 29), name="sweep_%08x" % zlib.crc32(case["id"].encode()))
        data = make_data(sp, 9000 + zlib.crc32(case["id"].encode()) % 100000, table_max=case.get("table_max", 3), nnz=case.get("nnz", (320, 8, 8)))
        if case.get("wide"):   # a WIDE row: `stock` keeps the integer weights its wide ones were drawn from
            data = dict(data, stock=data["ws"], ws=widen(case, data["ws"]))
        if case.get("records"):   # a RECORDS row: `stock_tables` / `stock_dense` keep the integers its preimages were drawn from
            data = wide_records(case, data)
        if case.get("f32w"):   # an F32_WIDTH row: carriers of a full fp32 significand in the record, the weights or both
            data = f32_width_data(case, data)
    else:
        sp = model_spec(case["model"])
        data = make_data(sp, model_seed(case["model"]))
    rng = np.random.default_rng(sum(map(ord, case["id"])))
    sel = rng.integers(0, data["idx"].shape[0], size=n_items)
    if case.get("f32w") in ("rec", "w1"):   # every position of P within the first |P| items
        sel = np.arange(n_items) % data["idx"].shape[0]
    dense = data["dense"][sel] if data["dense"] is not None else None
    if "stock_tables" in data:
        data = dict(data, sel=sel)
    return sp, data, data["idx"][sel], dense


def demangle(name):
    """'_Z17fc_lp_gemm_kernelILi0ELi1ELi128ELi2ELi8ELi32EEv...' or 'void fc_lp_gemm_kernel<0, 1, ...>(...)' -> 'fc_lp_gemm_kernel<0, 1, ...>'
    (the form fr_worker_last_kernel reports)."""
    if name.startswith("_Z"):
        m = re.match(r"_Z(\d+)", name)
        n = int(m.group(1))
        base, rest = name[m.end():m.end() + n], name[m.end() + n:]
        if not rest.startswith("I"):
            return base
        args = [(("true" if v == "1" else "false") if t == "b" else ("-" if neg else "") + v)
                for t, neg, v in re.findall(r"L([ib])(n?)(\d+)E", rest[1:rest.index("EE") + 1])]
        return "%s<%s>" % (base, ", ".join(args))
    return re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", name))


# ---- fp8 weight exponents from the weights (stats_kernel + floor_log2(448 / max|W|)) -------------------------------------------------------
TINY = (64, (64, 64, 64))   # K, hidden widths of the model the exponent tests run on


def _f32(v, toward=None):
    return np.float32(v) if toward is None else np.nextafter(np.float32(v), np.float32(toward))


# a layer's maximum |w| -> its exponent, worked out by hand: max * 2^e must land in (224, 448]
W_EXP_MAXIMA = [
    ("448", _f32(448), 0), ("448+", _f32(448, np.inf), -1), ("224", _f32(224), 1), ("224-", _f32(224, 0), 1), ("224+", _f32(224, np.inf), 0),
    ("3.5", _f32(3.5), 7), ("28", _f32(28), 4), ("27", _f32(27), 4), ("1", _f32(1), 8), ("2^-60", _f32(2.0 ** -60), 68), ("2^60", _f32(2.0 ** 60), -52),
]
W_EXP_PLACES = ("first", "last", "negative")


def layer_with_maximum(stock, m, place):
    """A layer of the stock weights' pattern scaled to |w| <= m / 2, with the maximum m at the first or the last element, or -m in the middle."""
    w = (np.asarray(stock, np.float32) * (np.float32(m) / np.float32(4.0))).ravel().copy()
    pos, val = {"first": (0, m), "last": (w.size - 1, m), "negative": (w.size // 2 + 1, -m)}[place]
    w[pos] = val
    assert (np.abs(np.delete(w, pos)) < np.abs(np.float32(m))).all()
    return w.reshape(np.shape(stock)), pos


# ---- the refresh sequence: every call that must rebuild a derived weight image, on one context --------------------------------------------
# ("prec", p): fr_ctx_set_fc_precision; ("set", l, which): fr_ctx_set_weights of layer l.  A and B are integer weight sets of two seeds
# (rounding is the WIDE rows' job, this is about staleness); A8 / A4 = A times 8 / 4, so that the fp8 weight exponent of the layer moves.
REFRESH_OPS = [("prec", "f32"), ("prec", "bf16"), ("set", 0, "B"), ("set", 1, "B"), ("set", 2, "B"), ("set", 3, "B"), ("prec", "fp8"),
               ("set", 1, "A8"), ("prec", "f32"), ("set", 2, "A4"), ("prec", "bf16"), ("prec", "fp8")]
REFRESH_SHAPES = {"pipeline": dict(K=112, fc=(256, 512, 256), batch=33, group=1), "fused": dict(K=352, fc=(1024, 512, 256), batch=64, group=16)}


def refresh_data(shape):
    s = REFRESH_SHAPES[shape]
    sp = spec(s["K"], s["fc"], name="refresh_" + shape)
    dA, dB = make_data(sp, 4101 + s["K"]), make_data(sp, 5202 + s["K"])
    sets = {"A": dA["ws"], "B": dB["ws"], "A8": [w * np.float32(8) for w in dA["ws"]], "A4": [w * np.float32(4) for w in dA["ws"]]}
    return sp, dA, sets


def refresh_steps(sets, precs=PRECS):
    """The sequence as (op, precision in force, the weights in force, stale candidates): a stale candidate is the weight list a context
    would compute with if it had left one layer's image of that precision as it was when the precision was last in force (or, after a
    set_weights, as it was before the call).  Ops of a precision outside `precs` are skipped (the CPU back-end: fp32 only)."""
    cur, prec = list(sets["A"]), "f32"
    seen = {p: list(cur) for p in PRECS}   # per precision, the weights its images were last built from
    out = []
    for op in REFRESH_OPS:
        if op[0] == "prec":
            if op[1] not in precs:
                continue
            prec = op[1]
        else:
            cur = list(cur)
            cur[op[1]] = sets[op[2]][op[1]]
        stale = []
        for l in range(4):
            if seen[prec][l] is not cur[l]:
                old = list(cur)
                old[l] = seen[prec][l]
                stale.append((l, old))
        seen[prec] = list(cur)
        out.append((op, prec, list(cur), stale))
    return out


# ---- the record side: records that must round, one row per reader of a record ---------------------------------------------------------------
# The stock tables and dense features are integers, exact in bf16 and in e4m3 at any power-of-two scale, so no conversion of a RECORD to the
# operand type ever rounds.  wide_records() replaces every table and dense value v by a float32 preimage of the operand-type image of
# v * 2^s under the chain's record conversion (bf16: RNE; e4m3: x 2^act_exp[0], clamp to +-448, RNE), drawn in turn from the witness classes
# of the image's preimage interval: both ties (where the interval holds them: an even significand), the float32 neighbours just inside each
# end, the value itself, values further inside; where the image is a power of two the lower ties and near-ties carry into its binade.  Zeros
# stay zeros and every other one is -0.0 (fp8: some are the tie 2^-10 that flushes to zero, or lie just inside it).  The rounded record is
# the stock record times 2^s, so premise() and the expectation are inherited: the scores are the stock scores times 2^s.  In fp8 the
# activation exponents are set explicitly, every one to the stock one minus s: the e4m3 image of the record (and of every hidden activation,
# which is 2^s larger in real units too) is the stock image bit for bit.  A `clamp` row sets the stock layer-0 exponent two above the calibrated one, so that the stock image holds the top
# code 448 (|v| >= 2 of the stock range 3): there, and only there, the preimages include values above 448, which the clamp brings back.
REC_S = {"bf16": 8, "fp8": 3}
BF16_CLASSES = ("tie toward zero", "just inside it", "three quarters toward it", "the value", "a quarter past it", "just inside the outer tie", "tie away from zero")
FP8_CLASSES = BF16_CLASSES + ("above 448 (clamped)",)
FP8_ABOVE = (449.0, 460.0, 464.0, 500.0, 2.0 ** 20)   # 464 is the tie between 448 and the code a conversion without the clamp would take
FP8_ZEROS = (0.0, -0.0, 2.0 ** -10, -2.0 ** -10, _in(2.0 ** -10, 0), 2.0 ** -20)   # +-2^-10: half the smallest subnormal, a tie that flushes to zero


def bf16_preimage(t):
    """The float32 interval that RNE takes to the bf16 value t (nonzero, finite, exact in bf16): (end nearer zero, outer end, closed).  Both ends
    are ties; they belong to the interval where t's significand is even (closed), and neither does where it is odd."""
    u = np.ascontiguousarray(t, np.float32).view(np.uint32).astype(np.int64)
    sign, mag = u & 0x80000000, u & 0x7FFFFFFF
    assert ((u & 0xFFFF) == 0).all() and (mag > 0x8000).all() and (mag < 0x7F800000).all()
    f = lambda b: (sign | b).astype(np.uint32).view(np.float32)
    return f(mag - 0x8000), f(mag + 0x8000), ((mag >> 16) & 1) == 0


def bf16_record_preimages(t, cls):
    """Per element of t (bf16 values as float32, zeros allowed: they stay) the witness of class cls[i] (an index into BF16_CLASSES); a tie
    class of an open interval takes the neighbour just inside instead."""
    t = np.ascontiguousarray(t, np.float32)
    out = t.copy()
    nz = t != 0
    u = t[nz].view(np.uint32).astype(np.int64)
    sign, mag = u & 0x80000000, u & 0x7FFFFFFF
    closed = ((mag >> 16) & 1) == 0
    c = np.asarray(cls)[nz]
    off = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5, c == 6],
                    [np.where(closed, -0x8000, -0x7FFF), -0x7FFF, -0x6000, 0, 0x2000, 0x7FFF, np.where(closed, 0x8000, 0x7FFF)])
    out[nz] = (sign | (mag + off)).astype(np.uint32).view(np.float32)
    return out


def _e4m3_quantum(a):
    _, ex = np.frexp(a)
    return np.ldexp(1.0, np.maximum(ex - 1, -6) - 3)


def e4m3_preimage(a):
    """The interval of magnitudes that clamp-then-RNE takes to the e4m3 magnitude a (0 < a <= 448, float64): (lower end, upper end, closed).
    The spacing below a power of two above 2^-6 is half the spacing above it; the top code 448 takes everything above it too (inf)."""
    a = np.asarray(a, np.float64)
    q = _e4m3_quantum(a)
    assert (a > 0).all() and (a <= 448).all() and (np.mod(a, q) == 0).all()
    m, _ = np.frexp(a)
    q_lo = np.where((m == 0.5) & (a > 2.0 ** -6), q / 2, q)
    return a - q_lo / 2, np.where(a == 448.0, np.inf, a + q / 2), np.mod(a / q, 2) == 0


def fp8_record_preimages(img, cls, rng):
    """Per element of img (e4m3 values, the stock record image in the scaled domain) a float32 witness of class cls[i] (FP8_CLASSES) in the
    same domain; class 7 applies where |img| == 448 only (elsewhere: the value).  Zeros draw from FP8_ZEROS."""
    img = np.asarray(img, np.float64)
    out = np.zeros(img.shape, np.float32)
    z = img == 0
    out[z] = np.array(FP8_ZEROS, np.float32)[rng.permutation(int(z.sum())) % len(FP8_ZEROS)]
    a = np.abs(img[~z])
    c = np.asarray(cls)[~z]
    lo, hi, closed = e4m3_preimage(a)
    hi_f = np.where(np.isinf(hi), a + _e4m3_quantum(a) / 2, hi)   # 448: 464 is no tie under the clamp, yet every value up to it (and past it) is a preimage
    lo32, hi32 = lo.astype(np.float32), hi_f.astype(np.float32)
    assert (lo32 == lo).all() and (hi32 == hi_f).all()
    lo_in, hi_in = np.nextafter(lo32, np.float32(np.inf)), np.nextafter(hi32, np.float32(0))
    top = a == 448.0
    above = np.array(FP8_ABOVE, np.float32)[rng.permutation(a.size) % len(FP8_ABOVE)]
    w = np.select([c == 0, c == 1, c == 2, c == 3, c == 4, c == 5, c == 6, (c == 7) & top],
                  [np.where(closed, lo32, lo_in), lo_in, (a - 0.75 * (a - lo)).astype(np.float32), a.astype(np.float32),
                   (a + 0.25 * (hi_f - a)).astype(np.float32), hi_in, np.where(closed | top, hi32, hi_in), above], default=a.astype(np.float32))
    out[~z] = np.copysign(w, img[~z]).astype(np.float32)
    return out


def record_exponent(row):
    """The layer-0 activation exponent of a row's STOCK fp8 data: the calibrated floor_log2(448 / (2 max|v|)), plus 2 on a `clamp` row."""
    return floor_log2_f32(np.float32(448.0) / (np.float32(2.0) * np.float32(row.get("table_max", 3)))) + (2 if row.get("clamp") else 0)


def _wide_values(v, prec, s, e0, rng):
    """Stock integers v -> their float32 preimages (see the head of this part)."""
    v = np.ascontiguousarray(v, np.float32)
    flat = v.ravel()
    ncls = len(BF16_CLASSES if prec == "bf16" else FP8_CLASSES)
    cls = rng.permutation(flat.size) % ncls
    if prec == "bf16":
        out = bf16_record_preimages(flat * np.float32(2.0 ** s), cls)
        z = np.flatnonzero(flat == 0)
        out[z[1::2]] = np.float32(-0.0)
    else:
        img = e4m3_image(flat * np.float32(2.0 ** e0))
        out = fp8_record_preimages(img, cls, rng) * np.float32(2.0 ** (s - e0))
    return out.reshape(v.shape)


def wide_records(row, data):
    """The row's data with every table and dense value replaced by a preimage; stock_tables / stock_dense keep the integers."""
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()) + 77)
    prec, s, e0 = row["prec"], REC_S[row["prec"]], record_exponent(row)
    tables = [_wide_values(t, prec, s, e0, rng) for t in data["tables"]]
    dense = _wide_values(data["dense"], prec, s, e0, rng) if data["dense"] is not None else None
    return dict(data, stock_tables=data["tables"], stock_dense=data["dense"], tables=tables, dense=dense)


def record_image(prec, rec, e_x=0, mode="rne"):
    """The operand-type image (float64, the domain FC1 sums in) of float32 records: bf16, or e4m3 of rec * 2^e_x; mode as bf16_image / e4m3_image."""
    if prec == "bf16":
        return bf16_image(rec, mode).astype(np.float64)
    return e4m3_image(np.asarray(rec, np.float32) * np.float32(2.0 ** e_x), mode)


def record_witnesses(prec, rec, e_x=0):
    """Of float32 records: dict of counts -- values the conversion must round, ties resolved toward zero / away from it, near-ties (one float32
    step inside a tie), roundings that carry into the next binade, negative zeros; fp8 also ties that flush to zero and values above 448."""
    v = np.asarray(rec, np.float32) * np.float32(2.0 ** (e_x if prec == "fp8" else 0))
    a, b = np.abs(v.astype(np.float64)), np.abs(record_image(prec, rec, e_x))
    if prec == "bf16":
        lowbits = np.ascontiguousarray(v).view(np.uint32) & 0xFFFF
        tie, near = lowbits == 0x8000, (lowbits == 0x7FFF) | (lowbits == 0x8001)
    else:
        q = _e4m3_quantum(a)
        tie = (a <= 448.0) & (np.mod(a, q) == q / 2)
        stepped = [np.abs(np.nextafter(np.abs(v), np.float32(d)).astype(np.float64)) for d in (0, np.inf)]
        near = (a <= 448.0) & ~tie & ((np.mod(stepped[0], _e4m3_quantum(stepped[0])) == _e4m3_quantum(stepped[0]) / 2) |
                                      (np.mod(stepped[1], _e4m3_quantum(stepped[1])) == _e4m3_quantum(stepped[1]) / 2))
    out = {"inexact": int((a != b).sum()), "tie toward zero": int((tie & (b < a)).sum()), "tie away": int((tie & (b > a)).sum()), "near-tie": int(near.sum()),
           "carry": int(((b > a) & (np.frexp(b)[1] > np.frexp(a)[1]) & (a > 0) & (b > 2.0 ** -6 if prec == "fp8" else True)).sum()),
           "-0.0": int(((v == 0) & np.signbit(v)).sum())}
    if prec == "fp8":
        out["flush tie"] = int((a == 2.0 ** -10).sum())
        out["above 448"] = int((a > 448.0).sum())
    return out


def _rec_row(tag, prec, K, fc, batch, layer, kernel, reader, width=1, group=1, dense_len=0, **kw):
    return dict(id="rec-%s-%s" % (prec, tag), spec=(K, tuple(fc), dense_len), prec=prec, batch=batch, width=width, group=group, layer=layer,
                kernel=kernel, reader=reader, records=True, **kw)


def _record_rows():
    """One row per precision for each distinct reader of a record (fr_api.cpp: fused_launch's kernels, pipeline_step's stage 0 / stage 1 forms and
    its GEMM launches, launch_fc's and fc_from_slices_impl's converters, the gather | out launch, the operand-type bank image), on the shape of
    the smallest CASES / SWEEPS / WIDE entry that reaches it.  `layer` as for WIDE; `fc_only`: fr_worker_fc_only also runs (records_to_*_kernel);
    `sharded`: the row is fr_worker_fc_from_slices on a two-shard context (frk_transpose_slices + q4_to_lp_kernel); `bank`: a per-bank context,
    run with the operand-type bank image on and off (the large-batch gather reads the image: convert_rows_lp_kernel made it)."""
    A, C = (1024, 512, 256), C_FC
    H, F8 = "fr_fused_tile_h_kernel<2, 2, %s>", "fr_fused_tile_f8_kernel<%d>"
    rows = [
        _rec_row("fused_h22", "bf16", 352, A, 256, "stream", H % "22, true, 16, 2", "chunked fused kernel, straight-line K = 352", group=16),
        _rec_row("fused_h55", "bf16", 880, A, 256, "stream", H % "55, false, 12, 2", "chunked fused kernel, K = 880, dense block mid-record", group=16, dense_len=16),
        _rec_row("hs22", "bf16", 352, A, 256, "stream", _hs_kernel(352), "persistent fused kernel, 22 k-groups", group=64),
        _rec_row("hs33", "bf16", 528, A, 200, "stream", _hs_kernel(528), "persistent fused kernel, 33 k-groups", group=16),
        _rec_row("hs33-below", "bf16", 368, A, 65, "stream", _hs_kernel(368), "persistent fused kernel, 23 of 33 k-groups: zero k-groups beside values that round", group=16),
        _rec_row("hs44", "bf16", 704, A, 200, "stream", _hs_kernel(704), "persistent fused kernel, 44 k-groups, dense block mid-record", group=16, dense_len=16),
        _rec_row("hs55", "bf16", 880, A, 256, "stream", _hs_kernel(880), "persistent fused kernel, 55 k-groups, dense block mid-record", group=128, dense_len=16),
        _rec_row("k16", "bf16", 112, (256, 512, 256), 33, "FC1", PIPE % (1, 1), "stage 1's q8 gather, K % 32 == 16"),
        _rec_row("fused_f6", "fp8", 352, A, 256, "stream", F8 % 6, "fp8 fused kernel, K = 352", group=16),
        _rec_row("fused_f14", "fp8", 880, A, 100, "stream", F8 % 14, "fp8 fused kernel, K = 880, dense block mid-record", group=16, dense_len=16),
        _rec_row("fused_f6-clamp", "fp8", 352, A, 256, "stream", F8 % 6, "fp8 fused kernel: records above 448 at the layer-0 scale", group=16, clamp=True),
        _rec_row("kpad", "fp8", 104, (256, 512, 256), 33, "FC1", PIPE % (1, 2), "stage 1's q16 gather, K % 64 == 40: zero K padding beside values that round"),
        _rec_row("kpad-dense", "fp8", 4200, C, 33, "FC1", PIPE % (1, 2), "stage 1's q16 gather, K % 64 == 40, dense block mid-record", dense_len=8),
    ]
    for prec in ("bf16", "fp8"):
        p = _PI[prec]
        k3 = 192 if prec == "bf16" else 384
        rows += [
            _rec_row("stages", prec, 3968, C, 65, "stages", None, "stage pipeline: gather-only step, stage 1, the multi-stage launch; dense block mid-record", group=4, dense_len=16),
            _rec_row("n128", prec, k3, C, 4090, "FC1", PPN % p, "large-batch transposing gather + records_to_%s_kernel in front of the 128 x 256 tiles" % ("q8_bf16" if p == 1 else "q16_fp8"), fc_only=True),
            _rec_row("slices", prec, 352, A, 256, "slices", None, "q4_to_lp_kernel<%d> behind frk_transpose_slices (fc_from_slices)" % p, sharded=True),
            _rec_row("gather_out", prec, 3968, R_FC, 4096, "gather_out", "fr_gather_out_kernel<%d>" % p, "gather | output layer in one launch", dense_len=16),
            _rec_row("image", prec, 3968, C, 4096, "FC1", PPN % p, "large-batch gather of a per-bank context: operand-type bank image on and off", dense_len=16, bank=True),
        ]
    rows.append(_rec_row("stages-clamp", "fp8", 3968, C, 65, "stages", None, "stage pipeline: records above 448 at the layer-0 scale", group=4, dense_len=16, clamp=True))
    return rows


RECORDS = _record_rows()
# Readers of a record that no RECORDS row reaches, with the reason (the coverage table of tests/test_exact_chain_cpu.py prints them).
RECORDS_LEFT_OUT = {
    "fr_fused_tile_hs_kernel reading operand-type rows (SRC = 1)": "frk_fused_hk_takes_lp_rows() is false in the product build: no fused kernel reads the bank image; "
                                                                   "the fused rows still run with fr_ctx_set_lp_bank_image on and off and must not change",
    "gather_pooled_kernel's operand-store arms, transpose_slices_lp_kernel": "pooled and table-sharded low-precision transports: tests/gather_matrix.py and tests/exact_sharded.py own them",
}


def record_row_exponents(row, stock_rec, ws):
    """(stock activation exponents, those the row sets): calibrated on the stock integers (+2 at layer 0 on a clamp row); each minus s.  (The
    record is the stock record times 2^s in real units, and so is every hidden activation: with all four exponents s lower every e4m3 image
    of the chain is the stock image bit for bit.  Layer 0's alone would leave R1 2^s too large for its stock exponent.)"""
    ae = act_exponents(stock_rec, ws)
    assert ae[0] + (2 if row.get("clamp") else 0) == record_exponent(row), (ae, row["id"])
    ae[0] = record_exponent(row)
    return ae, [e - REC_S["fp8"] for e in ae]


def stock_records(model, data, idx):
    """The stock integer records of a RECORDS row's items (data as case_data returned it)."""
    dense = data["stock_dense"][data["sel"]] if data["stock_dense"] is not None else None
    return records(model, dict(data, tables=data["stock_tables"]), idx, dense)


# ---- fp32 operand width: rows whose operands need the whole fp32 significand ------------------------------------------------------------------
# Every fp32 operand of the stock data is an integer of at most 11 significant bits: an fp32 kernel that read a bf16 / e4m3 row image, kept
# R1 in a narrower type or fed the MFMA a truncated operand would still be bit-exact.  Integer data cannot be stretched to 24 bits and still
# sum exactly in any order unless the wide term is alone in its sum, so the rows are built from CARRIERS: odd integers m, 2^22 <= |m| < 3 * 2^22 (from 2^23 on they need all 24 bits of the significand).
#   `rec`  record carriers (operand A of FC1, then R1 -> R2 -> R3 as operand A of the later layers).  A set P of record positions -- every
#          residue of k modulo the row's `kstep`, the first and the last K step, every table, the dense block -- may hold a carrier.  Each item of
#          the pool holds exactly ONE, at the position P[item % |P|] (its table row there is a carrier row; every other table row it reads, and
#          its dense block elsewhere, is in {-1, 0, 1}).  Position p has a chain of columns n_p of W1, j_p of W2, i_p of W3 with weight +-1
#          down to Wout[i_p] = +-1; the carrier rows of W1 (and the rows n_p of W2, j_p of W3, i_p of Wout) are zero elsewhere, so every
#          column of every layer takes at most one wide input, plus narrow ones.  Every partial sum is an integer below 2^24 (premise(),
#          unchanged), and every item's score is +-m plus a narrow sum: a 24-bit integer that has been operand A of all four layers.
#   `w1`   weight carriers (operand B of FC1), the mirror image: W1[p, n_p] = m_p, the item's record is +-1 at its own position of P and 0 at
#          the others; the chain below is the same.
#   `ulp`  operand B of FC2, FC3 and the output layer: a 24-bit weight there would need activations in {0, +-1}, which the chain cannot
#          promise, so (as wide_wout) the layer's weights are w * (1 + 2^-j) on shrunk data (WOUT_SHRINK), j as large as premise() still
#          passes and never below 12 -- no operand of 8 (bf16) or 11 (fp16, tf32) significant bits holds it.  One layer at a time (the quanta
#          of two such layers would multiply): the row runs three weight sets, ulp_weights(data, l) for l = 1, 2, 3.
F32_KINDS = ("rec", "w1", "ulp")
ULP_J_MIN = 12
ULP_NNZ = (2, 2, 2)   # nonzeros per column of W1, W2, W3 on an `ulp` row (where K > N the cover of every row sets the floor)


def _layout(sp):
    """Record position -> (table, column), table -1 = the dense block (Model.from_spec's segment order)."""
    out, dl, at = [], sp.get("dense_len", 0), sp.get("dense_at", 0)
    for t in range(len(sp["tables"]) + 1):
        if dl and t == at:
            out += [(-1, j) for j in range(dl)]
        if t < len(sp["tables"]):
            out += [(t, c) for c in range(sp["tables"][t]["dim"])]
    return out


def carrier_positions(sp, kstep):
    """P: one record position per residue modulo kstep, spread over the K steps (residue 0 in the first, kstep - 1 in the last), then one per
    table not yet hit (its middle column) and one in the dense block."""
    lay = _layout(sp)
    K = len(lay)
    steps = (K + kstep - 1) // kstep
    P = []
    for r in range(min(kstep, K)):
        g = 0 if r == 0 else steps - 1 if r == kstep - 1 else (r * 7) % steps
        k = g * kstep + r
        P.append(k if k < K else (g - 1) * kstep + r)
    if max(P) < (steps - 1) * kstep:   # K is no multiple of the step: the last, partial step takes a position of its own
        P.append(K - 1)
    hit = {lay[k][0] for k in P}
    for t in [-1] * bool(sp.get("dense_len", 0)) + list(range(len(sp["tables"]))):
        if t not in hit:
            ks = [k for k in range(K) if lay[k][0] == t]
            P.append(ks[len(ks) // 2])
    assert len(set(P)) == len(P)
    return P


def f32_width_data(row, data):
    """The data of an F32_WIDTH row (see the head of this part), from the stock data of its shape drawn with tables in {-1, 0, 1}.  Adds `active`
    (per pool item, its position of P), `P`, `chain` (per p: n_p, j_p, i_p) and, on an `ulp` row, `ulp_j` (the j reached per layer 1..3)."""
    kind = row["f32w"]
    if kind == "ulp":   # weights in {-1, 0, 1}: with the dense output layer (256 nonzeros) every magnitude counts against j
        data = dict(data, ws=[np.sign(w) for w in data["ws"]])
        js = {l: ulp_j(data, l) for l in (1, 2, 3)}
        return dict(data, stock=data["ws"], ulp_j=js)
    sp, fc = data["spec"], data["fc"]
    rng = np.random.default_rng(zlib.crc32(row["id"].encode()) + 5)
    lay = _layout(sp)
    P = carrier_positions(sp, row["kstep"])
    n_pool = data["idx"].shape[0]
    assert len(P) <= n_pool
    # |m| odd in [2^22, 3 * 2^22): 23 significant bits below 2^23, the full 24 from there on (a sum may add 2^22 of narrow terms and stay below 2^24)
    odd = lambda n: ((rng.integers(2 ** 21, 3 * 2 ** 21, size=n) * 2 + 1) * rng.choice([-1, 1], size=n)).astype(np.float32)
    tables = [t.copy() for t in data["tables"]]
    dense = data["dense"].copy() if data["dense"] is not None else None
    idx = data["idx"].copy()
    by_table = {}
    for p in P:
        by_table.setdefault(lay[p][0], []).append(p)
    # table t: its first 2 * |P_t| rows are carrier rows (row r carries at P_t[r % |P_t|]); the rest hold no carrier.  `fill`: what a row holds at
    # a position of P that is not its own -- anything narrow on a `rec` row, 0 on a `w1` row (the wide weight must meet one +-1 per item)
    n_carrier = {}
    for t, Pt in by_table.items():
        cols = [lay[p][1] for p in Pt]
        if t < 0:
            if kind == "w1":
                dense[:, cols] = 0.0
            continue
        n_carrier[t] = 2 * len(Pt)
        assert n_carrier[t] + 8 <= tables[t].shape[0], (t, n_carrier[t], tables[t].shape)
        if kind == "w1":
            tables[t][:, cols] = 0.0
        for r in range(n_carrier[t]):
            tables[t][r, cols[r % len(Pt)]] = odd(1)[0] if kind == "rec" else rng.choice([-1.0, 1.0])
    active = np.empty(n_pool, np.int64)
    for i in range(n_pool):
        p = P[i % len(P)]
        active[i] = p
        for t, nc in n_carrier.items():   # rows without a carrier for every table ...
            idx[i, t] = nc + idx[i, t] % (tables[t].shape[0] - nc)
        t, c = lay[p]
        if t < 0:
            dense[i, c] = odd(1)[0] if kind == "rec" else rng.choice([-1.0, 1.0])
        else:                              # ... but the item's own
            Pt = by_table[t]
            idx[i, t] = Pt.index(p) + len(Pt) * ((i // len(P)) % 2)
    ws = [w.copy() for w in data["ws"]]
    cols = [rng.permutation(fc[l + 1])[:len(P)] for l in range(3)]
    assert all(len(c) == len(P) for c in cols), (len(P), fc)
    sgn = lambda: float(rng.choice([-1.0, 1.0]))
    ws[0][P, :] = 0.0
    for l in (1, 2):
        ws[l][cols[l - 1], :] = 0.0
    ws[3][cols[2], :] = 0.0
    wide_w = odd(len(P))
    for q, p in enumerate(P):
        ws[0][p, cols[0][q]] = sgn() if kind == "rec" else wide_w[q]
        ws[1][cols[0][q], cols[1][q]] = sgn()
        ws[2][cols[1][q], cols[2][q]] = sgn()
        ws[3][cols[2][q], 0] = sgn()
    return dict(data, tables=tables, dense=dense, idx=idx, ws=ws, active=active, P=P, chain=[c.tolist() for c in cols])


def ulp_weights(data, l):
    """The weight set of an `ulp` row's run for layer l (1 = FC2, 2 = FC3, 3 = the output layer): layer l times (1 + 2^-j)."""
    ws = list(data["stock"])
    ws[l] = (ws[l] * np.float32(1.0 + 2.0 ** -data["ulp_j"][l])).astype(np.float32)
    return ws


def f32_runs(row, data):
    """(what, the layer widened or None, weights) of an F32_WIDTH row's runs: one, or the three layers of an `ulp` row in turn."""
    if row["f32w"] == "ulp":
        return [("layer %d x (1 + 2^-%d): " % (l, data["ulp_j"][l]), l, ulp_weights(data, l)) for l in (1, 2, 3)]
    return [("", None, data["ws"])]


def ulp_j(data, l):
    """The largest j <= 22 for which the chain with layer l's weights times (1 + 2^-j) keeps premise() on the whole pool: every product a multiple
    of the layer's quantum, every sum of |products| below 2^24 quanta, in layer l and in every layer behind it."""
    sp = data["spec"]
    lay = _layout(sp)
    rec = np.empty((data["idx"].shape[0], len(lay)), np.float32)
    for k, (t, c) in enumerate(lay):
        rec[:, k] = data["dense"][:, c] if t < 0 else data["tables"][t][data["idx"][:, t], c]
    acts, _ = fp32_acts(rec, data["ws"])
    for j in range(22, ULP_J_MIN - 1, -1):
        W = (data["ws"][l] * np.float32(1.0 + 2.0 ** -j)).astype(np.float64)
        x, ok = acts[l], True
        for L in range(l, 4):
            WL = W if L == l else data["ws"][L].astype(np.float64)
            la, lw = _lowbit(x), _lowbit(WL)
            ok = ok and la is not None and float((np.abs(x) @ np.abs(WL)).max()) < 2.0 ** (24 + la + lw)
            x = x @ WL
        if ok:
            return j
    raise AssertionError("no j >= %d keeps the premise for layer %d" % (ULP_J_MIN, l))


def _f32_row(tag, kind, K, fc, batch, layer, kernel, reader, kstep=32, group=1, dense_len=0):
    return dict(id="f32w-%s-%s" % (tag, kind), spec=(K, tuple(fc), dense_len), prec="f32", batch=batch, width=1, group=group, layer=layer, kernel=kernel,
                reader=reader, f32w=kind, kstep=kstep, table_max=1, rows=80, **({"nnz": ULP_NNZ} if kind == "ulp" else {}))


def _f32_rows():
    """Per fp32 reader (fr_api.cpp: fused_launch's fp32 kernels, pipeline_step's stages and GEMM launches, the gather | out launch) one row of
    each kind, on the shape of the CASES / SWEEPS entry that reaches it.  `layer` as for WIDE."""
    A = (1024, 512, 256)
    readers = [
        ("fused44", 352, A, 256, "stream", "fr_fused_tile_kernel<2, 44, 4, false>", "straight-line fused kernel, K = 352", dict(group=16)),
        ("fused110", 880, A, 200, "stream", "fr_fused_tile_kernel<2, 110, 2, false>", "straight-line fused kernel, K = 880, dense block mid-record", dict(group=16, dense_len=16)),
        ("fused_db", 512, A, 128, "stream", FUSED % (2, "true"), "generic-K fused kernel, double-buffered R1", dict(group=16)),
        ("fused_sb", 256, A, 128, "stream", FUSED % (2, "false"), "generic-K fused kernel, single R1 buffer", dict(group=16)),
        ("m2", 352, A, 256, "stream", "fr_fused_tile_m2_kernel<44>", "two-tile fused kernel", dict(group=64)),
        ("stages-split", 640, (384, 512, 256), 200, "stages", None, "stage pipeline, stages 1-4, a split-K plan with a split layer", dict(kstep=64)),
        ("stages-whole", 576, (384, 384, 256), 200, "stages", None, "stage pipeline, stages 1-4, no layer split", dict(kstep=64)),
        ("n128", 64, C_FC, 4090, "FC1", LP % (0, 2, 128, 2), "128 x 256 GEMM tiles (FC1)", {}),
        ("t64", 512, (192, 256, 256), 5500, "FC1", LP % (0, 1, 64, 2), "64 x 128 GEMM tiles (FC1, N = 192)", {}),
        ("t128", 96, C_FC, 1638, "FC1", LP % (0, 1, 128, 2), "128 x 128 GEMM tiles (FC1)", {}),
        ("gather_out", 3968, C_FC, 4096, "gather_out", "fr_gather_out_kernel<0>", "gather | output layer in one launch, dense block mid-record", dict(dense_len=16)),
    ]
    return [_f32_row(tag, kind, K, fc, batch, layer, kernel, reader, **kw) for tag, K, fc, batch, layer, kernel, reader, kw in readers for kind in F32_KINDS]


F32_WIDTH = _f32_rows()
F32_LEFT_OUT = {
    "transpose_slices_lp_kernel (the table-sharded re-pack)": "a low-precision transport in front of the fp32 chain: tests/exact_sharded.py owns the sharded path",
    "the pooled forms (gather_pooled_kernel's operand stores)": "sums of rows, not a reader of one record: tests/gather_matrix.py owns them",
}

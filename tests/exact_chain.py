"""Integer-valued FC-chain data on which every kernel must match the host bit for bit (helpers only; the tests are
tests/test_exact_chain_cpu.py and tests/test_gpu_exact_chain.py).

Tables and dense features are integers in [-3, 3], weights integers in {-2 .. 2}, sparse enough that no layer's sum of |products|
reaches 2^24 times the products' common power-of-two quantum (premise(), asserted before any comparison).  Every fp32 partial sum is
then exact in any order and any split, bf16 / e4m3 products are exact in fp32, the fp8 scales are powers of two: the only roundings
left are the chain's explicit ones (bf16 RNE per hidden layer; e4m3 clamp to +-448 then RNE), which the host restates
(gpu_helpers.chain_bf16_reference / chain_fp8_reference).  So there is no tolerance: one wrong column, k-group or tile shows."""
import re

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


def make_data(model_spec, seed, n_pool=256):
    """-> dict: tables (list of float32 [rows][dim]), ws (4 float32 [K][N] arrays, == column-major N x K flattened), fc, and a pool
    of n_pool items (idx int32 [n][n_tables], dense float32 [n][dense_len] or None)."""
    rng = np.random.default_rng(seed)
    fc = [sum(t["dim"] for t in model_spec["tables"]) + model_spec.get("dense_len", 0)] + list(model_spec["fc"]) + [1]
    vals = np.arange(-3, 4, dtype=np.float32)
    pv = np.array([0.02, 0.03, 0.05, 0.1, 0.2, 0.25, 0.35])   # mostly positive: FC1 sums of several hundred (bf16 / e4m3 must round)
    tables = [rng.choice(vals, size=(t["rows"], t["dim"]), p=pv).astype(np.float32) for t in model_spec["tables"]]
    ws = [_sparse_layer(rng, fc[0], fc[1], min(fc[0], 320), positive=True), _sparse_layer(rng, fc[1], fc[2], 8),
          _sparse_layer(rng, fc[2], fc[3], 8), _sparse_layer(rng, fc[3], 1, 12)]
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


def w_exponents(ws):
    """fp8 weight exponents floor_log2(448 / max|W|), in float32."""
    return [floor_log2_f32(np.float32(448.0) / np.float32(np.abs(ws[l]).max())) for l in range(3)]


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
    ops.append((x, ws[3].astype(np.float64)))
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
    """(spec, data, idx, dense) of a case: n_items rows drawn (with repetition) from its model's pool."""
    sp = model_spec(case["model"])
    data = make_data(sp, model_seed(case["model"]))
    rng = np.random.default_rng(sum(map(ord, case["id"])))
    sel = rng.integers(0, data["idx"].shape[0], size=n_items)
    dense = data["dense"][sel] if data["dense"] is not None else None
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

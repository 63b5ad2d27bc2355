"""The integer-valued exact-chain data (tests/exact_chain.py) on a machine without a GPU: the exactness premise holds for every case of the
GPU matrix, the CPU back-end matches the exact reference bit for bit, the exact comparison rejects simulated kernel bugs that the old
max-norm tolerances let through, and every FC-chain kernel compiled into libfleetrec.so is either named by a GPU-matrix case or listed
as unreachable.  For the shape sweep (exact_chain.SWEEPS: each kernel at the edges of the range its dispatch predicate accepts) the same
premise and witnesses per row, the CPU back-end on every fp32 row, per edge a simulated bug that must change a score of every row that
targets the edge, hashes that pin the existing matrix's data, and the printed coverage table.  For the master-weight side
(exact_chain.WIDE, W_EXP_MAXIMA, REFRESH_OPS): premise, hidden-layer and weight witnesses per row, the pack / Wout-form / exponent / stale-image
mutants, and the fp32 steps of the refresh sequence on the CPU back-end.  For the record side (exact_chain.RECORDS, F32_WIDTH): the preimage
helpers against brute force, premise, operand equality with the stock data and witness classes per row, the conversion / layout / width
mutants with their summaries, the CPU back-end on every fp32 width row, and the coverage table of readers."""
import os
import shutil
import sys

import numpy as np
import pytest

import exact_chain as E
from gpu_helpers import ROOT, bf16_round, e4m3_decode_table, e4m3_encode

_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_cache():
    """The cached models and data go when the module is done (not at interpreter shutdown, when the library handle is gone)."""
    yield
    _CACHE.clear()


def _case_rec(fr, case, n=None):
    key = (case["id"], n)
    if key not in _CACHE:
        sp, data, idx, dense = E.case_data(case, n or min(case["batch"], 512))
        m = fr.Model.from_spec(sp)
        _CACHE[key] = (m, data, idx, dense, E.records(m, data, idx, dense))
    return _CACHE[key]


@pytest.mark.parametrize("case", E.CASES, ids=[c["id"] for c in E.CASES])
def test_premise_holds_for_every_gpu_case(fr, case):
    """Every product a multiple of the layer's quantum, every sum of |products| below 2^24 quanta; the low-precision chains round (and
    meet exact ties) in every hidden layer; exponents and scores are deterministic."""
    m, data, idx, dense, rec = _case_rec(fr, case)
    ws = data["ws"]
    assert m.record_len == data["fc"][0] and list(m.fc) == data["fc"]
    for l in range(4):   # every k row and every output column of every layer has a nonzero weight
        assert (ws[l] != 0).any(axis=1).all() and (ws[l] != 0).any(axis=0).all()
    ae = we = None
    if case["prec"] == "fp8":
        ae, we = E.act_exponents(rec, ws), E.w_exponents(ws)
        assert we == [7, 7, 7]
        for l, a in enumerate(E.fp32_acts(rec, ws)[0]):   # max|act| * 2^e lands in (112, 224]: one binade of headroom below 448
            assert 112.0 < np.abs(a).max() * 2.0 ** ae[l] <= 224.0
    E.premise(case["prec"], rec, ws, ae, we)
    if case["prec"] != "f32":
        for l, (inexact, ties) in enumerate(E.rounding_witnesses(case["prec"], rec, ws, ae, we)):
            assert inexact > 0 and ties > 0, (case["id"], l, inexact, ties)
    s1 = E.expected(case["prec"], rec, ws, ae, we)
    sp, data2, idx2, dense2 = E.case_data(case, idx.shape[0])
    assert np.array_equal(idx2, idx) and all(np.array_equal(a, b) for a, b in zip(data2["ws"], ws))
    assert np.array_equal(E.expected(case["prec"], E.records(m, data2, idx2, dense2), data2["ws"], ae, we), s1)
    assert np.isfinite(s1).all() and np.unique(s1).size > s1.size // 4


@pytest.mark.parametrize("case_id", ["f32-A352-g16", "f32-C-b200", "f32-N192-5500", "f32-G256"])
def test_cpu_backend_bit_exact(fr, O, case_id):
    """The library's CPU back-end (fp32) on the exact data: every item bit for bit, and the oracle's fp64-accumulating chain agrees."""
    case = next(c for c in E.CASES if c["id"] == case_id)
    m, data, idx, dense, rec = _case_rec(fr, case, 96)
    want = E.expected("f32", rec, data["ws"])
    ctx = fr.Context(m, device=fr.DEVICE_CPU)
    try:
        E.load(ctx, data)
        wk = fr.Worker(ctx, idx.shape[0])
        got = wk.infer(idx, dense)
        assert np.array_equal(got, want)
        assert np.array_equal(wk.fc_scores(rec), want)
        wk.close()
    finally:
        ctx.close()
    assert np.array_equal(O.OracleModel("A").fc_chain(rec, [w.ravel() for w in data["ws"]], acc64=True, dims=data["fc"]), want)


# ---- mutants: known kernel bugs restated in numpy ------------------------------------------------------------------------------------

def _bf16_chain(rec, ws, x_hook=None, r_hook=None, w_hook=None, round3=True):
    x = bf16_round(rec).astype(np.float64)
    if x_hook:
        x = x_hook(x)
    for l in range(3):
        W = bf16_round(ws[l]).astype(np.float64)
        if w_hook:
            W = w_hook(l, W)
        r = (x @ W).astype(np.float32)
        if r_hook:
            r = r_hook(l, r)
        x = (bf16_round(r) if (l < 2 or round3) else r).astype(np.float64)
    return (x @ bf16_round(ws[3]).astype(np.float64)).astype(np.float32).ravel()


def _fp8_chain(rec, ws, ae, we, q_hook=None):
    dec = e4m3_decode_table()
    x = dec[e4m3_encode(rec * np.float32(2.0 ** ae[0]))]
    for l in range(3):
        Wf = dec[e4m3_encode(ws[l] * np.float32(2.0 ** we[l]))]
        r = ((x @ Wf) * 2.0 ** -(ae[l] + we[l])).astype(np.float32)
        x = dec[e4m3_encode(r * np.float32(2.0 ** ae[l + 1]))]
        if q_hook:
            x = q_hook(l, x)
    return ((x * 2.0 ** -ae[3]) @ ws[3].astype(np.float64)).astype(np.float32).ravel()


def _drop_kgroup(x):
    x = x.copy()
    x[-32:, 8:16] = 0.0          # FC1's k-group 1 missing for the last 32-item tile
    return x


def _wrong_column(l, r):
    if l == 0:
        r = r.copy()
        r[:, 3] += np.float32(1.0)   # one hidden output column off by one unit
    return r


def _swap_k(l, W):
    if l == 0:
        W = W.copy()
        col = 5
        nz = np.flatnonzero(W[:, col])
        k1 = nz[0]
        k2 = next(k for k in range(W.shape[0]) if W[k, col] != W[k1, col])
        W[[k1, k2], col] = W[[k2, k1], col]
    return W


def _saturate_one(l, x):
    if l == 1:
        x = x.copy()
        i, j = np.unravel_index(np.argmax(np.abs(x) * (np.abs(x) < 448)), x.shape)
        x[i, j] = 448.0 * np.sign(x[i, j])   # one R2 value clamped to the e4m3 maximum
    return x


MUTANTS = {
    "FC1 k-group dropped (last 32-item tile)": ("bf16", lambda rec, ws, ae, we: _bf16_chain(rec, ws, x_hook=_drop_kgroup)),
    "one FC1 output column off by one": ("bf16", lambda rec, ws, ae, we: _bf16_chain(rec, ws, r_hook=_wrong_column)),
    "FC3 not rounded to bf16": ("bf16", lambda rec, ws, ae, we: _bf16_chain(rec, ws, round3=False)),
    "two k swapped in one W1 column": ("bf16", lambda rec, ws, ae, we: _bf16_chain(rec, ws, w_hook=_swap_k)),
    "one fp8 R2 value saturated": ("fp8", lambda rec, ws, ae, we: _fp8_chain(rec, ws, ae, we, q_hook=_saturate_one)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_exact_comparison_rejects_mutant(fr, name):
    """Each simulated bug changes at least one score of the Model-C-shaped case data, so the bit-exact comparison rejects it; its max-norm
    error is printed next to the tolerance the precision's score tests allow (the mutant table of the change's description)."""
    prec, fn = MUTANTS[name]
    case = next(c for c in E.CASES if c["id"] == "%s-C-b65" % prec)
    m, data, idx, dense, rec = _case_rec(fr, case, 256)
    ws = data["ws"]
    ae, we = (E.act_exponents(rec, ws), E.w_exponents(ws)) if prec == "fp8" else (None, None)
    want = E.expected(prec, rec, ws, ae, we)
    bad = fn(rec, ws, ae, we)
    assert not np.array_equal(bad, want), name
    err = float(np.abs(bad.astype(np.float64) - want).max() / np.abs(want).max())
    print("mutant %-42s %-4s items changed %4d  max-norm err %.2e  old tolerance %.0e  %s" % (
        name, prec, int((bad != want).sum()), err, E.OLD_TOL[prec], "caught" if err > E.OLD_TOL[prec] else "MISSED by the tolerance"))


def test_exponent_check_rejects_act_exp2_off_by_one(fr):
    """A calibration that measures R2 without the binade of headroom (act_exp[2] one too large) returns an exponent vector that differs
    from the predicted one, which the GPU tests compare with ctx.fp8_exponents() item for item.  Its scores alone would not show it: a
    power-of-two scale one binade off changes no e4m3 rounding short of saturation or subnormals (printed below)."""
    case = next(c for c in E.CASES if c["id"] == "fp8-C-b65")
    m, data, idx, dense, rec = _case_rec(fr, case, 256)
    ws = data["ws"]
    ae, we = E.act_exponents(rec, ws), E.w_exponents(ws)
    r2 = E.fp32_acts(rec, ws)[0][2]
    bad_ae = list(ae)
    bad_ae[2] = E.floor_log2_f32(np.float32(448.0) / np.float32(np.abs(r2).max()))
    assert bad_ae != ae, (bad_ae, ae)
    want, bad = E.expected("fp8", rec, ws, ae, we), _fp8_chain(rec, ws, bad_ae, we)
    print("mutant %-42s fp8  items changed %4d  (exponents %s for %s)" % ("act_exp[2] off by one", int((bad != want).sum()), bad_ae, ae))


def test_mutant_restatements_match_the_reference(fr):
    """The mutants' chain restatements without a mutation are the exact reference (so a rejected mutant is rejected for its bug)."""
    for prec in ("bf16", "fp8"):
        case = next(c for c in E.CASES if c["id"] == "%s-C-b65" % prec)
        m, data, idx, dense, rec = _case_rec(fr, case, 256)
        ws = data["ws"]
        if prec == "bf16":
            assert np.array_equal(_bf16_chain(rec, ws), E.expected("bf16", rec, ws))
        else:
            ae, we = E.act_exponents(rec, ws), E.w_exponents(ws)
            assert np.array_equal(_fp8_chain(rec, ws, ae, we), E.expected("fp8", rec, ws, ae, we))


# ---- the shape sweep (exact_chain.SWEEPS) -----------------------------------------------------------------------------------------------

def _exps(row, rec, ws):
    return (E.act_exponents(rec, ws), E.w_exponents(ws)) if row["prec"] == "fp8" else (None, None)


def test_sweep_table_is_well_formed():
    ids = [r["id"] for r in E.SWEEPS]
    assert len(set(ids)) == len(ids)
    assert not set(ids) & {c["id"] for c in E.CASES}
    for r in E.SWEEPS:
        assert r["layer"] in ("FC1", "FC2", "FC3", "stream") and r["kernel"] and r["edge"] and r["family"] in E.FAMILIES, r["id"]
        assert (r["layer"] == "stream") == (r["group"] >= 12), r["id"]     # smaller launch groups ride the stage pipeline
        assert r["batch"] <= 200 or r["spec"][0] <= 960, r["id"]
    assert {r["family"] for r in E.SWEEPS} == set(E.FAMILIES)


@pytest.mark.parametrize("row", E.SWEEPS, ids=[r["id"] for r in E.SWEEPS])
def test_premise_holds_for_every_sweep_row(fr, row):
    """As for the GPU matrix: the exactness premise, rounding witnesses on every hidden layer (the swept one included), deterministic data,
    finite scores with more than a quarter of them distinct."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    ws = data["ws"]
    K, fc, _ = row["spec"]
    assert m.record_len == K and list(m.fc) == [K] + list(fc) + [1] == data["fc"]
    for l in range(4):
        assert (ws[l] != 0).any(axis=1).all() and (ws[l] != 0).any(axis=0).all()
    ae, we = _exps(row, rec, ws)
    if row["prec"] == "fp8":
        assert we == [7, 7, 7]
    E.premise(row["prec"], rec, ws, ae, we)
    if row["prec"] != "f32":
        for l, (inexact, ties) in enumerate(E.rounding_witnesses(row["prec"], rec, ws, ae, we)):
            assert inexact > 0 and ties > 0, (row["id"], l, inexact, ties)
    s1 = E.expected(row["prec"], rec, ws, ae, we)
    sp, data2, idx2, dense2 = E.case_data(row, idx.shape[0])
    assert np.array_equal(idx2, idx) and all(np.array_equal(a, b) for a, b in zip(data2["ws"], ws))
    assert all(np.array_equal(a, b) for a, b in zip(data2["tables"], data["tables"]))
    assert np.array_equal(E.expected(row["prec"], E.records(m, data2, idx2, dense2), data2["ws"], ae, we), s1)
    assert np.isfinite(s1).all() and np.unique(s1).size > s1.size // 4


F32_SWEEPS = [r for r in E.SWEEPS if r["prec"] == "f32"]


@pytest.mark.parametrize("row", F32_SWEEPS, ids=[r["id"] for r in F32_SWEEPS])
def test_cpu_backend_bit_exact_on_sweep(fr, row):
    """The library's CPU back-end on every fp32 sweep shape (at most 96 items): bit for bit."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 96))
    want = E.expected("f32", rec, data["ws"])
    ctx = fr.Context(m, device=fr.DEVICE_CPU)
    try:
        E.load(ctx, data)
        wk = fr.Worker(ctx, idx.shape[0])
        assert np.array_equal(wk.infer(idx, dense), want)
        wk.close()
    finally:
        ctx.close()


def _chain(prec, rec, ws, ae=None, we=None, prod=None):
    """The chain of precision `prec` with layer l's matrix product replaced by prod(l, A, W) on the operands the device multiplies
    (exact_chain.operands); prod None is the reference itself (asserted for every row before its mutants run)."""
    prod = prod or (lambda l, A, W: A @ W)
    if prec == "fp8":
        dec = e4m3_decode_table()
        x = dec[e4m3_encode(np.asarray(rec, np.float32) * np.float32(2.0 ** ae[0]))]
        for l in range(3):
            Wf = dec[e4m3_encode(ws[l] * np.float32(2.0 ** we[l]))]
            r = (prod(l, x, Wf) * 2.0 ** -(ae[l] + we[l])).astype(np.float32) * np.float32(2.0 ** ae[l + 1])
            x = dec[e4m3_encode(r)]
        return ((x * 2.0 ** -ae[3]) @ ws[3].astype(np.float64)).astype(np.float32).ravel()
    rnd = (lambda v: v) if prec == "f32" else bf16_round
    x = rnd(np.asarray(rec, np.float32)).astype(np.float64)
    for l in range(3):
        r = prod(l, x, rnd(ws[l]).astype(np.float64)).astype(np.float32)
        x = rnd(r).astype(np.float64)
    return (x @ rnd(ws[3]).astype(np.float64)).astype(np.float32).ravel()


def _at(L, fn):
    return lambda l, A, W: fn(A, W) if l == L else A @ W


def _drop_last_step(ks):
    def fn(A, W):
        k0 = (A.shape[1] + ks - 1) // ks * ks - ks
        return A[:, :k0] @ W[:k0]
    return fn


def _stale_stage(ks):
    return lambda A, W: A @ W - A[:, ks:2 * ks] @ W[ks:2 * ks] + A[:, :ks] @ W[:ks]


def _skip_chunk(c):
    def fn(A, W):
        A = A.copy()
        A[:, 256 * c:256 * (c + 1)] = 0.0
        return A @ W
    return fn


def _first_partial_only(A, W):
    h = A.shape[1] // 2
    return A[:, :h] @ W[:h]


def _pad_reads_last_group(g, kpad):
    def fn(A, W):
        K = A.shape[1]
        src = K - g + np.arange(kpad - K) % g
        return A @ W + A[:, src] @ W[src]
    return fn


def edge_mutants(row):
    """The simulated bugs at the edge a sweep row sits on: name -> prod hook of _chain."""
    L = 0 if row["layer"] == "stream" else ("FC1", "FC2", "FC3").index(row["layer"])
    KL = ([row["spec"][0]] + list(row["spec"][1]))[L]
    out = {}
    if row.get("kstep"):
        out["last K step of the swept layer dropped"] = _at(L, _drop_last_step(row["kstep"]))
        if KL > row["kstep"]:
            out["first K step used in place of the second (stale stage)"] = _at(L, _stale_stage(row["kstep"]))
    if row.get("chunks"):
        out["one H1 chunk of 256 skipped"] = _at(1, _skip_chunk(row["chunks"] - 1))   # FC2 never sees the last chunk of R1
    for l, ns in enumerate(row.get("split") or ()):
        if ns == 2:
            out["second split-K partial not added (FC%d)" % (l + 1)] = _at(l, _first_partial_only)
    if row.get("pad") and row["pad"][1] > KL:
        out["zero-padded k-groups read as the last real k-group"] = _at(L, _pad_reads_last_group(*row["pad"]))
    return out


@pytest.mark.parametrize("row", E.SWEEPS, ids=[r["id"] for r in E.SWEEPS])
def test_sweep_row_rejects_its_edge_mutants(fr, row):
    """Every mutant of the edge a row targets changes at least one of the row's scores: the data is not zero exactly where the edge bites."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    ws = data["ws"]
    ae, we = _exps(row, rec, ws)
    want = E.expected(row["prec"], rec, ws, ae, we)
    assert np.array_equal(_chain(row["prec"], rec, ws, ae, we), want)
    mutants = edge_mutants(row)
    assert mutants or row["family"] == "stage", row["id"]   # (a stage row of the unsplit plan (1, 1, 1) has no edge of its own to mutate)
    for name, prod in mutants.items():
        bad = _chain(row["prec"], rec, ws, ae, we, prod)
        assert not np.array_equal(bad, want), (row["id"], name)


def test_every_edge_mutant_is_exercised():
    names = set()
    for r in E.SWEEPS:
        names.update(n.split(" (FC")[0] for n in edge_mutants(r))
    assert names == {"last K step of the swept layer dropped", "first K step used in place of the second (stale stage)", "one H1 chunk of 256 skipped",
                     "second split-K partial not added", "zero-padded k-groups read as the last real k-group"}


# E.expected(...) of three cases of the GPU matrix (one per precision), sha256 of the float32 bytes, taken before SWEEPS and make_data's
# optional parameter existed: the sweep must not move the existing matrix's data.
PINNED = {
    "f32-A352-g16": "495c68bec55730a95c73061b56c1d8c7f367c2dbc931113d6f6755493173ed84",
    "bf16-C-b65": "304c361987611f31546af08843e6947b0988d9e29ef237ab90c0fc59e4f7bd1d",
    "fp8-C-b65": "e742c2656bd0594c736f7e8e359586333ab469e17df373bbc448be56696c41d4",
}


@pytest.mark.parametrize("case_id", list(PINNED))
def test_existing_matrix_did_not_move(fr, case_id):
    import hashlib
    case = next(c for c in E.CASES if c["id"] == case_id)
    m, data, idx, dense, rec = _case_rec(fr, case)
    ae, we = _exps(case, rec, data["ws"])
    s = E.expected(case["prec"], rec, data["ws"], ae, we)
    assert hashlib.sha256(np.ascontiguousarray(s, np.float32).tobytes()).hexdigest() == PINNED[case_id]


def test_sweep_coverage_table():
    """One line per kernel family: the range its predicate accepts, what the sweep covers, what it leaves out and why (printed; the table of the
    change's description)."""
    for fam, (accepted, omitted) in E.FAMILIES.items():
        rows = [r for r in E.SWEEPS if r["family"] == fam]
        assert rows, fam
        cover = sorted({"%s %s" % (r["prec"], r["cover"]) for r in rows})
        print("sweep %-8s %3d rows | accepts: %s | covers: %s | kernels: %s | left out: %s" % (
            fam, len(rows), accepted, ", ".join(cover), ", ".join(sorted({r["kernel"] for r in rows})), omitted))
    # the plans the stage rows and the GPU matrix give between them: every (partials read, own split) pair at FC2 and FC3
    pairs = {l: {(E.split_plan(r)[l - 1], E.split_plan(r)[l]) for r in E.SWEEPS if r["family"] == "stage" and r["prec"] == "f32"} for l in (1, 2)}
    assert pairs[1] | {(2, 2)} == pairs[2] | {(2, 2)} == {(1, 1), (1, 2), (2, 1), (2, 2)}, pairs   # (2, 2): Model C in the GPU matrix


# ---- kernel completeness -------------------------------------------------------------------------------------------------------------

def _fc_chain_kernels(fr):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    if not (os.path.exists(KR.READELF) or shutil.which("llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    names = {E.demangle(r["name"]) for r in KR.kernel_records(fr.LIB_PATH)}
    if not names:
        pytest.skip("no gfx950 code objects found in %s" % fr.LIB_PATH)
    return {n for n in names if n.startswith(("fr_fused_tile", "fr_pipeline_kernel", "fr_gather_out_kernel")) or (n.startswith("fc_") and "gemm" in n)}


def test_every_fc_chain_kernel_is_accounted_for(fr):
    """Each FC-chain kernel of libfleetrec.so is named by a GPU-matrix case or listed in UNREACHABLE with a reason -- and nothing else is."""
    lib = _fc_chain_kernels(fr)
    named = E.named_kernels()
    assert not (named & set(E.UNREACHABLE)), sorted(named & set(E.UNREACHABLE))
    assert sorted(lib - named - set(E.UNREACHABLE)) == [], "FC-chain kernels no GPU-matrix case names"
    assert sorted((named | set(E.UNREACHABLE)) - lib) == [], "names the library does not contain"
    assert all(E.UNREACHABLE.values())


def test_demangle():
    assert E.demangle("_Z17fc_lp_gemm_kernelILi0ELi1ELi128ELi2ELi8ELi32EEvPK15HIP_vector_typeIjLj4EES3_Pviiiiif") == "fc_lp_gemm_kernel<0, 1, 128, 2, 8, 32>"
    assert E.demangle("_Z18fr_pipeline_kernelILin1ELi2EEv10FrPipeArgs") == "fr_pipeline_kernel<-1, 2>"
    assert E.demangle("_Z20fr_fused_tile_kernelILi2ELi44ELi2ELb1EEv11FrFusedArgs") == "fr_fused_tile_kernel<2, 44, 2, true>"
    assert E.demangle("void fr_pipeline_kernel<-1, 0>(FrPipeArgs)") == "fr_pipeline_kernel<-1, 0>"


# ---- the master-weight side (exact_chain.WIDE, the exponent maxima, the refresh sequence) --------------------------------------------------

def _wide_exps(row, rec, ws):
    return (E.act_exponents(rec, ws), E.w_exponents(ws)) if row["prec"] == "fp8" else (None, None)


def test_wide_table_is_well_formed():
    ids = [r["id"] for r in E.WIDE]
    assert len(set(ids)) == len(ids) and not set(ids) & ({c["id"] for c in E.CASES} | {r["id"] for r in E.SWEEPS})
    shapes = {(c["prec"], E.MODELS[c["model"]][0], E.MODELS[c["model"]][1], c["batch"], c.get("width") or 1, c["group"]) for c in E.CASES}
    shapes |= {(r["prec"], r["spec"][0], r["spec"][1], r["batch"], r["width"], r["group"]) for r in E.SWEEPS}
    for r in E.WIDE:   # every row sits on the shape of an existing case or sweep row (a gather | out row: that of test_exact_gather_out_launch)
        assert (r["prec"], r["spec"][0], r["spec"][1], r["batch"], r["width"], r["group"]) in shapes, r["id"]
        assert r["prec"] in ("bf16", "fp8") and r["reader"]
    for prec in ("bf16", "fp8"):   # one row per precision for each distinct reader of a weight image
        readers = {r["kernel"] or r["layer"] for r in E.WIDE if r["prec"] == prec and not r["wout"]}
        p = E._PI[prec]
        assert {E.PPN % p, E.OUT % p, "fr_gather_out_kernel<%d>" % p, "stages", E.LP % (p, 1, 128, 2)} <= readers, readers
    assert {r["layer"] for r in E.WIDE if r["wout"]} == {"stream", "OUT", "FC3", "gather_out"}   # each output-layer implementation once


def test_preimage_pools_round_as_stated():
    """Every bf16 preimage rounds to its target, the values just outside the intervals do not; the e4m3 pool rounds as its comments say;
    the restated images agree with the reference's conversions."""
    for a, vals in E.BF16_PREIMAGES.items():
        v = np.array(vals, np.float32)
        assert (bf16_round(v) == 256.0 * a).all() and (bf16_round(-v) == -256.0 * a).all()
        assert bf16_round(np.nextafter(v[:1], np.float32(0)))[0] < 256.0 * a < bf16_round(np.nextafter(v[-1:], np.float32(1e9)))[0]
        assert len(vals) == 7 and len(set(vals)) == 7
    pool = np.array(E.FP8_POOL, np.float32)
    img = E.e4m3_image(pool * np.float32(16.0)) / 16.0
    assert img.tolist() == [16, 20, 20, 24, 24, 28, 16, 20, 20, 24, 28, 16, 16, 24, 28, 0]
    x = np.concatenate([np.random.default_rng(3).normal(0, 60, 4000), pool * 16, -pool, [0.0, 448.0, 449.0, -1e9, 2.0 ** -10, 3 * 2.0 ** -10]]).astype(np.float32)
    assert np.array_equal(E.e4m3_image(x), e4m3_decode_table()[e4m3_encode(x)])
    assert np.array_equal(E.bf16_image(x), bf16_round(x))
    for (top, s), want in zip(E.FP8_LAYERS, (3, 6, 7)):
        assert E.floor_log2_f32(np.float32(448.0) / np.float32(top * 2.0 ** s)) == want


@pytest.mark.parametrize("row", E.WIDE, ids=[r["id"] for r in E.WIDE])
def test_premise_holds_for_every_wide_row(fr, row):
    """Premise, hidden-layer witnesses as for the matrix, and per wide layer weights that are inexact, tie downward, tie upward and carry.
    bf16: the images are the stock images times a power of two, so the scores are the stock scores (the premise is inherited)."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    ws, stock, prec = data["ws"], data["stock"], row["prec"]
    ae, we = _wide_exps(row, rec, ws)
    for l in range(4):
        assert ((ws[l] != 0) == (stock[l] != 0)).all()
    if prec == "fp8" and not row["wout"]:
        assert we == [3, 6, 7]
        assert E.exponent_margin(E.act_exponent_quotients(rec, ws)) > 1e-3
    elif prec == "fp8":
        assert we == [7, 7, 7]
    E.premise(prec, rec, ws, ae, we)
    for l, (inexact, ties) in enumerate(E.rounding_witnesses(prec, rec, ws, ae, we)):
        assert inexact > 0 and ties > 0, (row["id"], l, inexact, ties)
    for l in row["wide"]:
        if prec == "fp8" and l == 3:   # the fp32 master: nine significant bits, so its bf16 image is another vector
            assert (E.bf16_image(ws[3])[ws[3] != 0] != ws[3][ws[3] != 0]).all()
        else:
            assert min(E.weight_witnesses(prec, l, ws[l], we)) > 0, (row["id"], l, E.weight_witnesses(prec, l, ws[l], we))
    s = E.expected(prec, rec, ws, ae, we)
    assert np.isfinite(s).all() and np.unique(s).size > s.size // 4
    if prec == "bf16":
        for l in range(4):
            assert np.array_equal(bf16_round(ws[l]), stock[l] * np.float32(2.0 ** (8 + E.BF16_SCALES[l])))
        assert np.array_equal(s, E.expected("bf16", rec, stock) * np.float32(2.0 ** (32 + sum(E.BF16_SCALES))))


def _image_chain(prec, rec, ws, ae, we, image=None, wout=None):
    """The chain with layer l's weight operand image(l) (None: the device's, exact_chain.weight_image) and the output layer's wout."""
    image = image or (lambda l: E.weight_image(prec, l, ws[l], we))
    Ws = [image(l) for l in range(3)] + [wout if wout is not None else image(3)]
    if prec == "fp8":
        dec = e4m3_decode_table()
        x = dec[e4m3_encode(np.asarray(rec, np.float32) * np.float32(2.0 ** ae[0]))]
        for l in range(3):
            r = ((x @ Ws[l]) * 2.0 ** -(ae[l] + we[l])).astype(np.float32) * np.float32(2.0 ** ae[l + 1])
            x = dec[e4m3_encode(r)]
        return ((x * 2.0 ** -ae[3]) @ Ws[3]).astype(np.float32).ravel()
    x = bf16_round(np.asarray(rec, np.float32)).astype(np.float64)
    for l in range(3):
        x = bf16_round((x @ Ws[l]).astype(np.float32)).astype(np.float64)
    return (x @ Ws[3]).astype(np.float32).ravel()


def weight_mutants(row, ws, we):
    """The simulated bugs of the master-weight side that a WIDE row targets: name -> (image hook, wout) of _image_chain."""
    prec, out = row["prec"], {}
    if row["wout"]:
        return {"fp8 chain with a bf16 Wout": (None, E.bf16_image(ws[3]).astype(np.float64))}
    for l in row["wide"]:
        def one(fn, l=l):
            return lambda k: fn(k) if k == l else E.weight_image(prec, k, ws[k], we)
        scaled = (lambda k: ws[k].astype(np.float64) * 2.0 ** we[k]) if prec == "fp8" else (lambda k: ws[k].astype(np.float64))
        out["%s pack truncates (layer %d)" % (prec, l)] = (one(lambda k: E.weight_image(prec, k, ws[k], we, "trunc")), None)
        out["%s pack rounds half away (layer %d)" % (prec, l)] = (one(lambda k: E.weight_image(prec, k, ws[k], we, "away")), None)
        out["layer %d reads the fp32 master instead of its %s image" % (l, prec)] = (one(scaled), None)
    if prec == "bf16":
        out["bf16 chain with an fp32 Wout"] = (None, ws[3].astype(np.float64))
    return out


@pytest.mark.parametrize("row", E.WIDE, ids=[r["id"] for r in E.WIDE])
def test_wide_row_rejects_its_weight_mutants(fr, row):
    """Truncation, round-half-away and master-instead-of-image in each wide layer, and the other form of Wout, each change a score of
    the row (the count is printed: the mutant table of the change's description); the unmutated restatement is the reference."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    ws, prec = data["ws"], row["prec"]
    ae, we = _wide_exps(row, rec, ws)
    want = E.expected(prec, rec, ws, ae, we)
    assert np.array_equal(_image_chain(prec, rec, ws, ae, we), want)
    mutants = weight_mutants(row, ws, we)
    assert len(mutants) == (1 if row["wout"] else 13 if prec == "bf16" else 9)
    for name, (image, wout) in mutants.items():
        bad = _image_chain(prec, rec, ws, ae, we, image, wout)
        err = float(np.nanmax(np.abs(bad.astype(np.float64) - want)) / np.abs(want).max())
        print("weight mutant %-32s %-58s items changed %4d of %d  max-norm err %.2e  old tolerance %.0e" % (
            row["id"], name, int((bad != want).sum()), want.size, err, E.OLD_TOL[prec]))
        assert not np.array_equal(bad, want), (row["id"], name)


def test_weight_exponent_restatement_and_its_mutants():
    """E.w_exponent against the exponents worked out by hand (max * 2^e in (224, 448]) for every maximum and placement of the GPU test;
    `max without abs` changes the exponent of every negative placement, `NaN drives the max` that of every layer with a NaN
    whose exponent is not 0, which is what the mutant gives (the GPU test's NaN layers have exponents 6, 7, 8)."""
    stock = E.make_data(E.spec(*E.TINY), 611, n_pool=8)["ws"]
    for name, m_val, by_hand in E.W_EXP_MAXIMA:
        assert 224.0 < float(m_val) * 2.0 ** by_hand <= 448.0, name
        for l in range(3):
            for place in E.W_EXP_PLACES:
                W, pos = E.layer_with_maximum(stock[l], m_val, place)
                assert E.w_exponent(W) == by_hand, (name, l, place)
                assert (E.w_exponent(W, use_abs=False) != by_hand) == (place == "negative"), (name, l, place)
                V = W.ravel().copy()
                V[pos + 1 if pos + 1 < V.size else pos - 1] = np.nan
                assert E.w_exponent(V) == by_hand and (E.w_exponent(V, skip_nan=False) != by_hand) == (by_hand != 0), (name, l, place)
    assert E.w_exponent(np.zeros(64, np.float32)) == 0
    for seed, scale in ((611, 1.0), (612, 0.37), (613, 5.0)):   # the uncalibrated estimates the GPU test reads back: clear of a binade edge
        d = E.make_data(E.spec(*E.TINY), seed, n_pool=8)
        assert E.exponent_margin(E.estimated_act_exponents([w * np.float32(scale) for w in d["ws"]], d["fc"])[1]) >= 0.01


@pytest.mark.parametrize("shape", list(E.REFRESH_SHAPES))
def test_refresh_sequence_on_the_host_and_the_cpu_back_end(fr, shape):
    """Every step of exact_chain.REFRESH_OPS on the host: the premise holds, the expected scores differ from the previous step's and from
    those of every stale-image mutant.  The fp32 steps then run on the CPU back-end, on a worker that lives through all of them and on a
    fresh one per step."""
    s = E.REFRESH_SHAPES[shape]
    sp, dA, sets = E.refresh_data(shape)
    m = fr.Model.from_spec(sp)
    idx = dA["idx"][:s["batch"]]
    rec = E.records(m, dA, idx, None)
    prev, ae, n_stale = None, None, 0
    for op, prec, ws, stale in E.refresh_steps(sets):
        we = E.w_exponents(ws) if prec == "fp8" else None
        if prec == "fp8" and op[0] == "prec":
            ae = E.act_exponents(rec, ws)
        E.premise(prec, rec, ws, ae, we)
        want = E.expected(prec, rec, ws, ae, we)
        assert prev is None or not np.array_equal(want, prev), op
        for l, old in stale:
            assert not np.array_equal(E.expected(prec, rec, old, ae, E.w_exponents(old)), want), (op, l)
            n_stale += 1
        prev = want
    assert n_stale >= 12
    ctx = fr.Context(m, device=fr.DEVICE_CPU)
    try:
        E.load(ctx, dA)
        live = fr.Worker(ctx, s["batch"])
        prev = None
        for op, prec, ws, stale in E.refresh_steps(sets, precs=("f32",)):
            if op[0] == "set":
                ctx.set_weights(op[1], ws[op[1]].ravel())
            want = E.expected("f32", rec, ws)
            assert op[0] == "prec" or not np.array_equal(want, prev), op   # (back to fp32 from fp32: the one step that changes nothing here)
            fresh = fr.Worker(ctx, s["batch"])
            assert np.array_equal(live.infer(idx, None), want) and np.array_equal(fresh.infer(idx, None), want), op
            fresh.close()
            prev = want
        live.close()
    finally:
        ctx.close()


# ---- the record side (exact_chain.RECORDS) and fp32 operand width (exact_chain.F32_WIDTH) ---------------------------------------------------

def _shapes():
    shapes = {(c["prec"], E.MODELS[c["model"]][0], E.MODELS[c["model"]][1], c["batch"], c.get("width") or 1, c["group"]) for c in E.CASES}
    return shapes | {(r["prec"], r["spec"][0], r["spec"][1], r["batch"], r["width"], r["group"]) for r in E.SWEEPS + E.WIDE}


def test_record_and_width_tables_are_well_formed():
    ids = [r["id"] for r in E.RECORDS + E.F32_WIDTH]
    assert len(set(ids)) == len(ids) and not set(ids) & ({c["id"] for c in E.CASES} | {r["id"] for r in E.SWEEPS + E.WIDE})
    shapes = _shapes()
    for r in E.RECORDS + E.F32_WIDTH:   # every row sits on the shape of an existing case or row (a `sharded` row: fc_from_slices on Model-A's shape)
        assert (r["prec"], r["spec"][0], r["spec"][1], r["batch"], r["width"], r["group"]) in shapes or r.get("sharded"), r["id"]
        assert r["reader"] and 33 <= r["batch"] <= (5500 if r["prec"] == "f32" else 4096), r["id"]   # (5500: the one shape with 64 x 128 fp32 tiles at FC1)
    for prec in ("bf16", "fp8"):   # one row per precision for each distinct reader of a record
        p = E._PI[prec]
        readers = {r["kernel"] or r["layer"] for r in E.RECORDS if r["prec"] == prec}
        assert {"stages", "slices", E.PPN % p, E.PIPE % (1, p), "fr_gather_out_kernel<%d>" % p} <= readers, readers
        assert any(r.get("bank") for r in E.RECORDS if r["prec"] == prec) and any(r.get("fc_only") for r in E.RECORDS if r["prec"] == prec)
        dense = {r["kernel"] or r["layer"] for r in E.RECORDS if r["prec"] == prec and r["spec"][2]}
        assert all(r["group"] == 4 for r in E.RECORDS if r["layer"] == "stages")   # several batches in flight: the multi-stage launch
        assert "stages" in dense and any(k.startswith("fr_fused_tile") for k in dense), dense   # a dense block mid-record for a fused and a pipeline reader
    bf = {r["kernel"] for r in E.RECORDS if r["prec"] == "bf16"}
    assert {E._hs_kernel(K) for K in (352, 528, 704, 880)} <= bf and "fr_fused_tile_h_kernel<2, 2, 22, true, 16, 2>" in bf
    assert {"fr_fused_tile_f8_kernel<6>", "fr_fused_tile_f8_kernel<14>"} <= {r["kernel"] for r in E.RECORDS if r["prec"] == "fp8"}
    assert any(r["spec"][0] % 64 == 40 for r in E.RECORDS if r["prec"] == "fp8") and any(r["spec"][0] % 32 == 16 for r in E.RECORDS if r["prec"] == "bf16")
    assert any(r.get("clamp") for r in E.RECORDS)
    tags = {r["id"].rsplit("-", 1)[0] for r in E.F32_WIDTH}   # each fp32 reader: one row of each kind
    for tag in tags:
        assert {r["f32w"] for r in E.F32_WIDTH if r["id"].rsplit("-", 1)[0] == tag} == set(E.F32_KINDS), tag
    named = {r["kernel"] or r["layer"] for r in E.F32_WIDTH}
    assert {"fr_fused_tile_kernel<2, 44, 4, false>", "fr_fused_tile_kernel<2, 110, 2, false>", E.FUSED % (2, "true"), E.FUSED % (2, "false"), "fr_fused_tile_m2_kernel<44>",
            "stages", E.LP % (0, 2, 128, 2), E.LP % (0, 1, 64, 2), E.LP % (0, 1, 128, 2), "fr_gather_out_kernel<0>"} == named, named
    plans = {r["id"]: E.split_plan(r) for r in E.F32_WIDTH if r["layer"] == "stages"}
    assert all(2 in plans["f32w-stages-split-" + k] and plans["f32w-stages-whole-" + k] == (1, 1, 1) for k in E.F32_KINDS), plans


def test_record_preimage_helpers_round_as_stated():
    """bf16_preimage against brute force: both ends are ties, they round to t exactly where t's significand is even, their float32 neighbours
    inside do always and those outside never; every class of bf16_record_preimages rounds to t.  The same for e4m3_preimage on all 126
    positive codes (the top one: no upper end) and for every class of fp8_record_preimages; FP8_ZEROS all flush to zero, FP8_ABOVE all clamp."""
    t = np.array([v * 2.0 ** s for v in range(1, 13) for s in (-3, 0, 8)] + [258.0, 262.0, 1.0078125, 129.0 * 2.0 ** -20, 255.0], np.float32)
    t = np.concatenate([t, -t])
    lo, hi, closed = E.bf16_preimage(t)
    assert closed[:36].all() and not closed[36:41].any()   # v < 16 times a power of two: an even significand; 258 = 129 * 2, ...: odd
    up = lambda v, d: np.nextafter(v, np.float32(d) * np.sign(v))
    assert ((bf16_round(lo) == t) == closed).all() and ((bf16_round(hi) == t) == closed).all()
    assert (bf16_round(up(lo, np.inf)) == t).all() and (bf16_round(up(hi, 0)) == t).all()
    assert (bf16_round(up(lo, 0)) != t).all() and (bf16_round(up(hi, np.inf)) != t).all()
    assert (np.abs(lo) < np.abs(t)).all() and (np.abs(t) < np.abs(hi)).all()
    for c in range(len(E.BF16_CLASSES)):
        w = E.bf16_record_preimages(t, np.full(t.size, c))
        assert (bf16_round(w) == t).all() and ((w == t) == (c == 3)).all(), c
    dec = e4m3_decode_table()
    a = dec[1:127]
    lo, hi, closed = E.e4m3_preimage(a)
    img = lambda v: E.e4m3_image(np.asarray(v, np.float32))
    assert np.isinf(hi[-1]) and a[-1] == 448.0
    lo32, hi32 = lo.astype(np.float32), hi[:-1].astype(np.float32)
    assert ((img(lo32) == a) == closed).all() and ((img(hi32) == a[:-1]) == closed[:-1]).all()
    assert (img(np.nextafter(lo32, np.float32(np.inf))) == a).all() and (img(np.nextafter(hi32, np.float32(0))) == a[:-1]).all()
    assert (img(np.nextafter(lo32, np.float32(0))) != a).all() and (img(np.nextafter(hi32, np.float32(np.inf))) != a[:-1]).all()
    rng = np.random.default_rng(5)
    both = np.concatenate([a, -a])
    for c in range(len(E.FP8_CLASSES)):
        w = E.fp8_record_preimages(both, np.full(both.size, c), rng)
        assert np.array_equal(E.e4m3_image(w), both), c
        assert np.array_equal(dec[e4m3_encode(w)], both), c
    assert (np.abs(E.fp8_record_preimages(np.array([448.0] * 20), np.full(20, 7), rng)) > 448).all()
    assert (E.e4m3_image(np.array(E.FP8_ZEROS, np.float32)) == 0).all() and (E.e4m3_image(np.array(E.FP8_ABOVE, np.float32)) == 448).all()
    assert E.e4m3_image(np.array([2.0 ** -10], np.float32), "away")[0] == 2.0 ** -9


def _record_row(fr, row, n=256):
    """(model, data, idx, dense, wide records, stock records, stock exponents, the row's exponents, w_exp)."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], n))
    stock = E.stock_records(m, data, idx)
    if row["prec"] == "fp8":
        ae_s, ae = E.record_row_exponents(row, stock, data["ws"])
        return m, data, idx, dense, rec, stock, ae_s, ae, E.w_exponents(data["ws"])
    return m, data, idx, dense, rec, stock, None, None, None


@pytest.mark.parametrize("row", E.RECORDS, ids=[r["id"] for r in E.RECORDS])
def test_premise_holds_for_every_record_row(fr, row):
    """premise() on the rounded operands; operands() of the wide data are those of the stock data times 2^s (bf16) or the same e4m3 images
    (fp8), layer for layer, so the scores are the stock scores times 2^s; every witness class is present in the batch's records (values above
    448 on a clamp row and nowhere else); no hidden activation comes near bf16's overflow or underflow."""
    m, data, idx, dense, rec, stock, ae_s, ae, we = _record_row(fr, row)
    ws, prec, s = data["ws"], row["prec"], E.REC_S[row["prec"]]
    assert np.isfinite(rec).all() and not np.array_equal(rec, stock)
    assert np.array_equal(rec == 0, stock == 0) or prec == "fp8"        # (fp8: some zeros are ties that flush)
    E.premise(prec, rec, ws, ae, we)
    ops, hidden = E.operands(prec, rec, ws, ae, we)
    ops_s, hidden_s = E.operands(prec, stock, ws, ae_s, we)
    f = 2.0 ** s if prec == "bf16" else 1.0
    for l in range(4):
        assert np.array_equal(ops[l][0], ops_s[l][0] * (f if prec == "bf16" or l < 3 else 2.0 ** s)), (row["id"], l)
        assert np.array_equal(ops[l][1], ops_s[l][1]), (row["id"], l)
    for r, x in hidden:
        nz = np.abs(r[r != 0])
        assert nz.max() < 2.0 ** 100 and nz.min() > 2.0 ** -100
    for l, (inexact, ties) in enumerate(E.rounding_witnesses(prec, rec, ws, ae, we)):
        assert inexact > 0 and ties > 0, (row["id"], l, inexact, ties)
    wit = E.record_witnesses(prec, rec, ae[0] if ae else 0)
    for k, n in wit.items():
        assert (n > 0) == (k != "above 448" or bool(row.get("clamp"))), (row["id"], wit)
    want = E.expected(prec, rec, ws, ae, we)
    assert np.array_equal(want, E.expected(prec, stock, ws, ae_s, we) * np.float32(2.0 ** s))
    assert np.isfinite(want).all() and np.unique(want).size > want.size // 4
    if row.get("clamp"):
        assert (np.abs(E.record_image("fp8", stock, ae_s[0])) == 448).any() and ae_s[0] == E.act_exponents(stock, ws)[0] + 2


def _from_image(prec, x0, ws, ae, we):
    """The chain of precision bf16 / fp8 from a given operand image of the records (float64, the domain FC1 sums in)."""
    if prec == "fp8":
        dec = e4m3_decode_table()
        x = x0
        for l in range(3):
            Wf = dec[e4m3_encode(ws[l] * np.float32(2.0 ** we[l]))]
            r = ((x @ Wf) * 2.0 ** -(ae[l] + we[l])).astype(np.float32) * np.float32(2.0 ** ae[l + 1])
            x = dec[e4m3_encode(np.nan_to_num(r))]
            x[np.isnan(r)] = np.nan   # (a mutant's NaN stays one)
        return ((x * 2.0 ** -ae[3]) @ ws[3].astype(np.float64)).astype(np.float32).ravel()
    x = x0
    for l in range(3):
        x = bf16_round((x @ bf16_round(ws[l]).astype(np.float64)).astype(np.float32)).astype(np.float64)
    return (x @ bf16_round(ws[3]).astype(np.float64)).astype(np.float32).ravel()


def _lane_perm(K, n, rot):
    k = np.arange(K)
    return (k // n) * n + (k % n + rot) % n


def record_mutants(row, rec, e_x):
    """The simulated bugs of a record's conversion and layout: name -> operand image of the records."""
    prec = row["prec"]
    n = 2 if prec == "bf16" else 4
    rne, trunc = E.record_image(prec, rec, e_x), E.record_image(prec, rec, e_x, "trunc")
    perm = _lane_perm(rec.shape[1], n, 1)
    step = np.where(rne != trunc, rne - trunc, 0.0)   # the rounding's own step up in magnitude, where it took one
    scaled = np.abs(np.asarray(rec, np.float32) * np.float32(2.0 ** e_x)).astype(np.float64)
    quantum = np.ldexp(1.0, np.frexp(np.maximum(np.abs(trunc), 2.0 ** -126))[1] - 8) if prec == "bf16" else E._e4m3_quantum(np.minimum(np.maximum(scaled, 2.0 ** -9), 448.0))
    took = (step != 0)[:, perm]
    out = {
        "record conversion truncates": trunc,
        "record conversion rounds half away from zero": E.record_image(prec, rec, e_x, "away"),
        "%s exchanged" % ("the two halves of a packed bf16 pair" if n == 2 else "e4m3 quad lanes rotated: positions"): rne[:, perm],
        "the rounding decision taken from the %s" % ("other half of the pair" if n == 2 else "next lane of the quad"): trunc + np.copysign(quantum, np.where(trunc == 0, rec, trunc)) * took,
    }
    if row.get("clamp"):   # a conversion that rounds first: past the tie 464 there is no finite code, the top one is taken only by what the clamp would have brought back
        bad = rne.copy()
        bad[scaled >= 464.0] = np.nan
        out["e4m3 rounding before the clamp"] = bad
    return out


RECORD_MUTANT_SHARES = {}


def _run_record_mutants(fr, row):
    if row["id"] not in RECORD_MUTANT_SHARES:
        RECORD_MUTANT_SHARES[row["id"]] = _record_mutants_of(fr, row)
    return RECORD_MUTANT_SHARES[row["id"]]


@pytest.mark.parametrize("row", E.RECORDS, ids=[r["id"] for r in E.RECORDS])
def test_record_row_rejects_its_record_mutants(fr, row):
    """Truncation, round-half-away, an exchanged pair / rotated quad (positions, and the rounding decision alone), and on a clamp row rounding
    before the clamp each change a score of the row; the unmutated restatement is the reference.  A -0.0 that becomes +0.0 changes no
    score and cannot: a sum with one nonzero term has no signed zero left, and no item's FC1 column is all zeros."""
    for name, (share, inside) in _run_record_mutants(fr, row).items():
        assert share > 0, (row["id"], name)


def _record_mutants_of(fr, row):
    m, data, idx, dense, rec, stock, ae_s, ae, we = _record_row(fr, row)
    out = {}
    ws, prec = data["ws"], row["prec"]
    e_x = ae[0] if ae else 0
    want = E.expected(prec, rec, ws, ae, we)
    assert np.array_equal(_from_image(prec, E.record_image(prec, rec, e_x), ws, ae, we), want)
    for name, img in record_mutants(row, rec, e_x).items():
        bad = _from_image(prec, img, ws, ae, we)
        changed = int((~(bad == want)).sum())
        err = float(np.nanmax(np.abs(bad.astype(np.float64) - want)) / np.abs(want).max()) if np.isfinite(bad).any() else np.inf
        inside = np.isfinite(bad).all() and err <= E.OLD_TOL[prec]
        out[name] = (changed / want.size, bool(inside))
        print("record mutant %-24s %-60s items changed %4d of %d  max-norm err %.2e  old tolerance %.0e%s" % (
            row["id"], name, changed, want.size, err, E.OLD_TOL[prec], "  INSIDE the old tolerance" if inside else ""))
    plus = E.record_image(prec, rec, e_x) + 0.0   # -0.0 + 0.0 = +0.0
    assert np.signbit(E.record_image(prec, rec, e_x)[rec == 0]).any() and not np.signbit(plus[plus == 0]).any()
    assert np.array_equal(_from_image(prec, plus, ws, ae, we), want)
    A, W = E.operands(prec, rec, ws, ae, we)[0][0]
    assert (np.abs(A) @ np.abs(W) > 0).all()
    return out


def test_record_mutant_summary(fr):
    """Per record mutant the least share of scores it changes over the rows that target it, and how many (mutant, row) pairs the old max-norm
    tolerances would have let through (printed: the table of the change's description)."""
    by_name = {}
    for row in E.RECORDS:
        for name, got in _run_record_mutants(fr, row).items():
            by_name.setdefault(name.replace("the two halves of a packed bf16 pair", "pair halves / quad lanes").replace("e4m3 quad lanes rotated: positions", "pair halves / quad lanes")
                               .replace("other half of the pair", "neighbouring lane").replace("next lane of the quad", "neighbouring lane"), []).append(got)
    for name, got in by_name.items():
        print("record mutant summary %-62s rows %2d  least share of scores changed %.3f  inside the old tolerance on %d rows" % (
            name, len(got), min(s for s, _ in got), sum(i for _, i in got)))
        assert min(s for s, _ in got) > 0


@pytest.mark.parametrize("row_id", ["rec-fp8-fused_f6", "rec-fp8-stages"])
def test_calibration_on_wide_records_is_certain(fr, row_id):
    """The rows the GPU calibration test runs: the fp32 chain's maxima on the WIDE records lie far from a power-of-two edge (the device sums
    these floats inexactly and in no fixed order), and the exponents calibrate must return are the stock ones minus s."""
    row = next(r for r in E.RECORDS if r["id"] == row_id)
    m, data, idx, dense, rec, stock, ae_s, ae, we = _record_row(fr, row, row["batch"])
    assert E.exponent_margin(E.act_exponent_quotients(rec, data["ws"])) > 1e-2
    assert E.act_exponents(rec, data["ws"]) == ae


def _round_bits(x, n):
    """x (float64) rounded to n significant bits, to nearest even."""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(np.ldexp(m, n)), e - n)


def _f32_chain(rec, ws, a_hook=None, w_hook=None):
    x = np.asarray(rec, np.float64)
    for l in range(4):
        W = ws[l].astype(np.float64)
        x = ((a_hook(l, x) if a_hook else x) @ (w_hook(l, W) if w_hook else W)).astype(np.float32).astype(np.float64)
    return x.astype(np.float32).ravel()


def _f32_runs(data, row):
    return E.f32_runs(row, data)


@pytest.mark.parametrize("row", E.F32_WIDTH, ids=[r["id"] for r in E.F32_WIDTH])
def test_premise_holds_for_every_f32_width_row(fr, row):
    """premise() unchanged.  Carrier rows: the positions P hit every residue of k modulo the row's K step, the first and the last step, every
    table and the dense block, and the batch's items use all of them; each item holds one carrier (rec) or one +-1 among zeros on P (w1); every
    column of every layer takes at most one wide input; the scores need more than 11 bits, and some all 24.  ulp rows: j >= 12 per layer."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    kind, K = row["f32w"], row["spec"][0]
    for what, l, ws in _f32_runs(data, row):
        E.premise("f32", rec, ws)
        s = E.expected("f32", rec, ws)
        assert np.isfinite(s).all() and np.unique(s).size > s.size // 4
        s64 = s.astype(np.float64)
        assert (_round_bits(s64, 11) != s64).mean() > 0.9, (row["id"], what)
        if l is not None:
            assert data["ulp_j"][l] >= E.ULP_J_MIN
            nz = ws[l][ws[l] != 0].astype(np.float64)
            assert (_round_bits(nz, 11) != nz).all() and (bf16_round(ws[l])[ws[l] != 0] != ws[l][ws[l] != 0]).all()
    if kind == "ulp":
        return
    P, ks, ws = data["P"], row["kstep"], data["ws"]
    lay = E._layout(data["spec"])
    assert {p % ks for p in P} == set(range(min(ks, K))) and min(P) < ks and max(P) >= (K - 1) // ks * ks
    assert {lay[p][0] for p in P} == set(range(m.n_tables)) | ({-1} if row["spec"][2] else set())
    active = data["active"][np.arange(idx.shape[0]) % data["active"].size]
    assert set(active.tolist()) == set(P)
    wide = np.abs(rec) >= 2.0 ** 22
    on_p = rec[:, P]
    if kind == "rec":
        assert (wide.sum(axis=1) == 1).all() and (np.argmax(wide, axis=1) == active).all() and (np.abs(rec[~wide]) <= 1).all()
        assert (rec[wide] % 2 == 1).all() and (np.abs(rec[wide]) >= 2.0 ** 23).any() and (np.abs(rec[wide]) < 2.0 ** 23).any()
        assert all(np.abs(w).max() <= 2 for w in ws)
    else:
        assert not wide.any() and (np.abs(rec) <= 1).all() and ((on_p != 0).sum(axis=1) == 1).all() and (np.abs(rec[np.arange(rec.shape[0]), active]) == 1).all()
        big = np.abs(ws[0]) >= 2.0 ** 22
        assert (big.sum(axis=0) <= 1).all() and (big.sum(axis=1)[P] == 1).all() and big.sum() == len(P) and (ws[0][big] % 2 == 1).all()
    acts, _ = E.fp32_acts(rec, ws)
    for l in range(4):   # at most one wide input per output column and item
        assert ((np.abs(acts[l] if l else (rec if kind == "rec" else np.zeros_like(rec))) >= 2.0 ** 21).astype(np.float64) @ (ws[l] != 0) <= 1).all(), (row["id"], l)
    s = E.expected("f32", rec, ws).astype(np.float64)
    assert (np.abs(s) >= 2.0 ** 21).all() and (_round_bits(s, 23) != s).any()


def f32_mutants(row, data, l_run):
    """The simulated narrow operands a row targets: name -> (a_hook, w_hook) of _f32_chain.  Operand A of layer l is the record (l = 0) or
    R_l, so `R_l stored at 11 bits` is the same arithmetic as `operand A of layer l at 11 bits` and is listed under both names."""
    kind, out = row["f32w"], {}
    rnd = {"bf16": lambda v: bf16_round(v.astype(np.float32)).astype(np.float64), "11 bits": lambda v: _round_bits(v, 11), "23 bits": lambda v: _round_bits(v, 23)}
    at = lambda L, fn: (lambda l, v: fn(v) if l == L else v)
    if kind == "rec":
        for L in range(4):
            for name, fn in rnd.items():
                out["operand A of layer %d rounded to %s" % (L, name)] = (at(L, fn), None)
            if L:
                out["R%d stored at 11 bits" % L] = (at(L, rnd["11 bits"]), None)
    elif kind == "w1":
        for name, fn in rnd.items():
            out["operand B of layer 0 rounded to %s" % name] = (None, at(0, fn))
    else:
        for name in ("bf16", "11 bits"):
            out["operand B of layer %d rounded to %s" % (l_run, name)] = (None, at(l_run, rnd[name]))
    return out


F32_MUTANT_SHARES = {}


@pytest.mark.parametrize("row", E.F32_WIDTH, ids=[r["id"] for r in E.F32_WIDTH])
def test_f32_width_row_rejects_its_width_mutants(fr, row):
    """Every narrow-operand mutant a row targets changes at least one of its scores (on a carrier row: rounding to 23 bits too)."""
    for name, (share, inside) in _run_f32_mutants(fr, row).items():
        assert share > 0, (row["id"], name)


def _run_f32_mutants(fr, row):
    if row["id"] in F32_MUTANT_SHARES:
        return F32_MUTANT_SHARES[row["id"]]
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 256))
    out = F32_MUTANT_SHARES.setdefault(row["id"], {})
    for what, l, ws in _f32_runs(data, row):
        want = E.expected("f32", rec, ws)
        assert np.array_equal(_f32_chain(rec, ws), want)
        for name, (a_hook, w_hook) in f32_mutants(row, data, l).items():
            bad = _f32_chain(rec, ws, a_hook, w_hook)
            changed = int((bad != want).sum())
            err = float(np.abs(bad.astype(np.float64) - want).max() / np.abs(want).max())
            out[name] = (changed / want.size, err <= E.OLD_TOL["f32"])
            print("width mutant %-26s %-44s items changed %4d of %d  max-norm err %.2e  old tolerance %.0e%s" % (
                row["id"], name, changed, want.size, err, E.OLD_TOL["f32"], "  INSIDE the old tolerance" if err <= E.OLD_TOL["f32"] else ""))
    return out


def test_f32_width_mutant_summary(fr):
    """Per width mutant the least share of scores it changes over the rows that target it, and on how many rows the old 1e-3 bar would have
    let it through (printed: the table of the change's description)."""
    by_name = {}
    for row in E.F32_WIDTH:
        for name, got in _run_f32_mutants(fr, row).items():
            by_name.setdefault(name, []).append(got)
    assert len(by_name) == 12 + 3 + 3 + 6
    for name, got in by_name.items():
        print("width mutant summary %-44s rows %2d  least share of scores changed %.3f  inside the old tolerance on %d rows" % (
            name, len(got), min(s for s, _ in got), sum(i for _, i in got)))
        assert min(s for s, _ in got) > 0


@pytest.mark.parametrize("row", E.F32_WIDTH, ids=[r["id"] for r in E.F32_WIDTH])
def test_cpu_backend_bit_exact_on_f32_width(fr, row):
    """The library's CPU back-end (fp32 too) on every F32_WIDTH row, at most 128 items: the same bits."""
    m, data, idx, dense, rec = _case_rec(fr, row, min(row["batch"], 128))
    ctx = fr.Context(m, device=fr.DEVICE_CPU)
    try:
        E.load(ctx, data)
        wk = fr.Worker(ctx, idx.shape[0])
        for what, l, ws in _f32_runs(data, row):
            for k in range(4):
                ctx.set_weights(k, ws[k].ravel())
            want = E.expected("f32", rec, ws)
            assert np.array_equal(wk.infer(idx, dense), want), (row["id"], what)
            assert np.array_equal(wk.fc_scores(rec), want), (row["id"], what)
        wk.close()
    finally:
        ctx.close()


def test_record_and_width_coverage_table():
    """For every reader of a record and every fp32 MFMA operand the row that pins it; what no row reaches, with the reason (printed)."""
    for r in E.RECORDS:
        print("record reader %-5s %-58s | %s | row %s%s" % (r["prec"], r["kernel"] or r["layer"], r["reader"], r["id"],
                                                           " (+ fr_worker_fc_only)" if r.get("fc_only") else " (bank image on and off)" if r.get("bank") else ""))
    for name, why in E.RECORDS_LEFT_OUT.items():
        print("record reader left out: %s -- %s" % (name, why))
    operands = {"rec": "operand A of FC1, FC2, FC3, output layer", "w1": "operand B of FC1", "ulp": "operand B of FC2, FC3, output layer (one run each)"}
    for r in E.F32_WIDTH:
        print("fp32 operand  %-42s | %s | %s | row %s" % (r["kernel"] or r["layer"], r["reader"], operands[r["f32w"]], r["id"]))
    for name, why in E.F32_LEFT_OUT.items():
        print("fp32 reader left out: %s -- %s" % (name, why))
    assert all(E.RECORDS_LEFT_OUT.values()) and all(E.F32_LEFT_OUT.values())

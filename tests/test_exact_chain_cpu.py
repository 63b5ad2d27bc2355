"""The integer-valued exact-chain data (tests/exact_chain.py) on a machine without a GPU: the exactness premise holds for every case of the
GPU matrix, the CPU back-end matches the exact reference bit for bit, the exact comparison rejects simulated kernel bugs that the old
max-norm tolerances let through, and every FC-chain kernel compiled into libfleetrec.so is either named by a GPU-matrix case or listed
as unreachable.  For the shape sweep (exact_chain.SWEEPS: each kernel at the edges of the range its dispatch predicate accepts) the same
premise and witnesses per row, the CPU back-end on every fp32 row, per edge a simulated bug that must change a score of every row that
targets the edge, hashes that pin the existing matrix's data, and the printed coverage table.  For the master-weight side
(exact_chain.WIDE, W_EXP_MAXIMA, REFRESH_OPS): premise, hidden-layer and weight witnesses per row, the pack / Wout-form / exponent / stale-image
mutants, and the fp32 steps of the refresh sequence on the CPU back-end."""
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

"""Factored request-form batches on the MI355X (reqfc_user_kernel + reqfc_cand_kernel of libfleetrec_reqfc.so, then stage 2 of the stage
pipeline): the checks of tests/request_factored.py on the device, in both chain precisions, and one run on float data."""
import numpy as np
import pytest

import exact_chain as E
import request_factored as F
import request_form as Q
from gpu_helpers import chain_bf16_reference

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "bias+relu"])
@pytest.mark.parametrize("shape", list(F.SHAPES))
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_exact_scores(fr, gpu, prec, shape, epi):
    F.check_shape(fr, gpu, prec, epi, shape)


def test_malformed_offsets(fr, gpu):
    """(Safe by construction: the owner is clamped, U / X_C / R1 are addressed inside ldm; the CPU twin of the same cases runs under ASan + UBSan:
    make -C csrc san-reqfc.)"""
    F.check_malformed(fr, gpu)


@pytest.mark.parametrize("which", F.REFUSALS)
def test_refusals(fr, gpu, which):
    F.check_refusal(fr, gpu, which)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_float_data(fr, gpu, prec):
    """Model-A's shape (352-float record, rows capped), seeded normal tables and weights, batch 64 of 4 requests, 20 of the 47 columns shared.
    Max-norm error against the float64-accumulating numpy chain on the expanded rows -- in bf16 the restatement with the chain's own roundings,
    the reference exact_chain.OLD_TOL is set against (tests/test_gpu_lowprec.py) -- under OLD_TOL; the full-row path's error is printed beside it."""
    rng = np.random.default_rng(2026)
    m = Q.model(fr, "A")
    ctx = fr.Context(m, device=gpu)
    try:
        fc = list(m.fc)
        tables = [rng.standard_normal((int(r), int(t.dim))).astype(np.float32) for r, t in zip(m.rows(), m.tables())]
        ws = [(rng.standard_normal((fc[l], fc[l + 1])) / np.sqrt(fc[l])).astype(np.float32) for l in range(4)]
        E.load(ctx, {"tables": tables, "ws": ws})
        ctx.set_fc_precision(fr.FC_BF16 if prec == "bf16" else fr.FC_FP32)
        shared = (np.arange(m.n_tables) < 20).astype(np.int32)
        ctx.set_request_columns(shared, False)
        wk = fr.Worker(ctx, 64)
        x = Q.Inputs(fr, rng, m, shared, False, 64, 4, off=np.arange(0, 65, 16))
        full = x.full.view(np.int32)
        rec = E.records(m, {"tables": tables}, full, x.dense)
        if prec == "bf16":
            ref = chain_bf16_reference(rec, [w.ravel() for w in ws], fc).ravel().astype(np.float64)
        else:
            ref = rec.astype(np.float64)
            for w in ws:
                ref = ref @ w.astype(np.float64)
            ref = ref.ravel()
        args = (x.req.view(np.int32), x.cand.view(np.int32), x.off)
        err = lambda s: float(np.abs(s.astype(np.float64) - ref).max() / np.abs(ref).max())
        e_fact, e_full = err(wk.infer_requests_factored(*args, dense=x.dense)), err(wk.infer_requests(*args, dense=x.dense, pooled=0))
        print("%s: max-norm error factored %.3e, full rows %.3e (bar %.0e)" % (prec, e_fact, e_full, E.OLD_TOL[prec]))
        assert e_fact <= E.OLD_TOL[prec]
        wk.close()
    finally:
        ctx.close()

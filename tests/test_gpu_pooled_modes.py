"""Pooling modes (FR_POOL_SUM / FR_POOL_MEAN) and per-sample weights of the multi-hot lookups on the MI355X: the weighted and the MEAN folds
of gather_pooled_kernel (csrc/fr_gather.hip) behind fr_ctx_set_pooling_modes and fr_worker_*_pooled_weighted*.  The same checks as
tests/test_cpu_pooled_modes.py (tests/pooled_modes.py states the contract in numpy), plus: fr_worker_last_kernel() is the case's own
instantiation in every weighted and MEAN gather (all eight run both folds), the narrow instantiation takes over when only the weight array
is off a 16-byte boundary, and the bf16 chain from weighted and MEAN records.

Bars: records bit-exact against the numpy fold wherever the expectation is not a NaN, a NaN where it is; scores bit-exact against
fr_worker_fc_only on the expected records (fp32 and bf16: the same chain from the same records); the hosts' printed scores against an
exact closed form.  No tolerance anywhere.  Every context here is a shrunk or a spec model."""
import pytest
from conftest import free_port_block

import gather_matrix as GM
import pooled_modes as PM

pytestmark = pytest.mark.gpu

MODES = {"table": 0, "item": 1, "bank": 2}   # fr.INDEX_PER_TABLE / PER_ITEM / PER_BANK
CASE_IDS = [c["id"] for c in GM.POOLED_CASES]


@pytest.mark.parametrize("what", ["weighted", "modes"])
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_pooled_case(fr, gpu, case_id, what):
    """Checks 1 and 2 on every case of gather_matrix.POOLED_CASES (the case's inputs are built once for both)."""
    (PM.run_case_weighted if what == "weighted" else PM.run_case_modes)(fr, gpu, case_id)


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank")])
def test_all_ones_weights_equal_the_unweighted_records(fr, gpu, kind, mode):
    PM.check_ones_identity(fr, gpu, kind, MODES[mode], B=1040 if kind == 2 else 70)


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_one_slot_mean_equals_gather_only(fr, gpu, kind, mode):
    PM.check_hots1_mean_is_gather_only(fr, gpu, kind, MODES[mode])


@pytest.mark.parametrize("kind,mode", [(0, "table"), (1, "bank"), ("spec", "table")])
def test_even_odd_known_answers(fr, gpu, kind, mode):
    PM.check_even_odd_known_answers(fr, gpu, kind, MODES[mode])


@pytest.mark.parametrize("kind,prec", [("spec", "f32"), (0, "f32"), (0, "bf16")])
def test_scores_from_weighted_and_mean_records(fr, gpu, kind, prec):
    PM.check_scores(fr, gpu, kind, precision=fr.FC_BF16 if prec == "bf16" else None)


@pytest.mark.parametrize("kind,mode", [(0, "table"), ("spec", "bank")])
def test_errors(fr, gpu, kind, mode):
    PM.check_errors(fr, gpu, kind, MODES[mode])


def test_sharded_contexts_refuse_pooling_modes(fr, gpu):
    PM.check_sharded_refuses_modes(fr, gpu)


@pytest.mark.parametrize("pool,ragged", [("weighted", False), ("weighted", True), ("mean", False), ("mean", True)])
def test_server_answers_weighted_and_mean_requests_on_the_gpu(fr, gpu, pool, ragged):
    PM.check_server(fr, gpu, pool, ragged, free_port_block)

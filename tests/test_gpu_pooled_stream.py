"""Streaming pushes of pooled lookups on the MI355X (tests/pooled_stream.py): the operand the pooled gather writes for stage 1, byte for byte
and pads included, in all eight shapes of gather_pooled_kernel and the three operand types; pushed scores against the submit form, bit for
bit, in fp32, bf16 and e4m3; one-hot and pooled pushes alternating through the stage pipeline and across the fused kernel; errors and state."""
import pytest

import gather_matrix as GM
import pooled_stream as PS

pytestmark = pytest.mark.gpu

# fp32: the mixed-width model (below one workgroup, one group) and the wide one (8 XCD groups); bf16 / e4m3: shrunk Model-A and the per-bank
# shrunk Model-C (the chains of `mixed` / `wide` are too narrow for fr_ctx_set_fc_precision: hidden widths of 32)
OPERAND = [("mixed", 0), ("wide", 0), ("A", 1), ("C", 1), ("A", 2), ("C", 2)]


@pytest.mark.parametrize("model,prec", OPERAND, ids=["%s-%s" % (m, ("fp32", "bf16", "e4m3")[p]) for m, p in OPERAND])
@pytest.mark.parametrize("kernel", list(GM.POOLED_HOTS), ids=[k[len("gather_pooled_kernel<"):-1].replace(", ", "-") for k in GM.POOLED_HOTS])
def test_operand_byte_for_byte(fr, kernel, model, prec):
    PS.check_operand(fr, 0, kernel, model, prec)


@pytest.mark.parametrize("kind,precision,caps_kind,mode", [
    (0, None, "spread", None), (0, None, "ones", None), (2, None, "five", "bank"),
    (0, 1, "spread", None), (2, 1, "ones", "bank"), (0, 2, "five", None), (2, 2, "spread", "bank")],
    ids=["A-fp32-spread", "A-fp32-ones", "C-fp32-five", "A-bf16-spread", "C-bf16-ones", "A-e4m3-five", "C-e4m3-spread"])
def test_pushed_scores_equal_the_submit_form(fr, kind, precision, caps_kind, mode):
    PS.check_scores_equal_submit(fr, 0, kind, precision, caps_kind, index_mode=fr.INDEX_PER_BANK if mode == "bank" else None)


@pytest.mark.parametrize("group", [8, None], ids=["group8-pipeline", "default-group-fused"])
def test_one_hot_and_pooled_pushes_alternate(fr, group):
    PS.check_mixing(fr, 0, group)


def test_update_rows_between_two_pooled_pushes(fr):
    PS.check_order_against_update_rows(fr, 0)


def test_range_errors_among_clean_batches(fr):
    PS.check_range_errors(fr, 0)


def test_state_and_arguments(fr):
    PS.check_state_and_arguments(fr, 0)


def test_host_fed_block_refuses(fr):
    PS.check_host_fed_block_refuses(fr, 0)

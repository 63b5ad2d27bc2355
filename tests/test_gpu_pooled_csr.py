"""The offsets (CSR) input form of the pooled lookups on the MI355X: the offsets arms of gather_pooled_kernel (csrc/fr_gather.hip) behind
fr_worker_gather_pooled_csr, fr_worker_submit_pooled_csr_device and fr_worker_submit_pooled_csr.  The same checks as
tests/test_cpu_pooled_csr.py (tests/pooled_csr.py), plus: fr_worker_last_kernel() is the NARROW instantiation of the window in every
offsets-form gather (also when every cap is a multiple of 4), and the bf16 and fp8 chains from offsets-form records.

Bars: records bit-exact, in every word, against the numpy fold and against the padded entry point on the same context, into guarded
destinations; scores bit-exact against the padded submit.  No tolerance anywhere.  Every context here is a shrunk or a spec model."""
import pytest
from conftest import free_port_block

import pooled_csr as PC

pytestmark = pytest.mark.gpu

MODES = {"table": 0, "item": 1, "bank": 2}
CASE_KINDS = [(c, k) for c in PC.CASE_IDS for k in PC.KINDS]


@pytest.mark.parametrize("case_id,kind", CASE_KINDS)
def test_csr_case(fr, gpu, case_id, kind):
    PC.run_case(fr, gpu, case_id, kind)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_caps_that_are_multiples_of_four_take_the_narrow_kernel(fr, gpu, kind):
    PC.run_case(fr, gpu, PC.CASE_CAPS4["id"], kind)


@pytest.mark.parametrize("case_id", [c for c in PC.CASE_IDS if "-mixed-" in c])
def test_arrays_off_a_16_byte_boundary(fr, gpu, case_id):
    PC.run_case(fr, gpu, case_id, "weighted", shifts=((4, 8, 12), (8, 12, 4), (12, 4, 8)), batches=(3, 37))


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_cap_one_bags_of_one_equal_gather_only(fr, gpu, kind, mode):
    PC.check_cap1_is_gather_only(fr, gpu, kind, MODES[mode])


@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("what", PC.MALFORMED)
def test_malformed_bag(fr, gpu, what, place):
    PC.check_malformed(fr, gpu, what, place)


@pytest.mark.parametrize("what", PC.MALFORMED)
def test_malformed_bag_under_weights(fr, gpu, what):
    PC.check_malformed(fr, gpu, what, "last", kind="weighted")


@pytest.mark.parametrize("kind,mode", [(0, "table"), ("spec", "bank")])
def test_errors(fr, gpu, kind, mode):
    PC.check_errors(fr, gpu, kind, MODES[mode])


def test_sharded_contexts_refuse_the_offsets_form(fr, gpu):
    PC.check_sharded_refuses(fr, gpu)


@pytest.mark.parametrize("kind,prec", [("spec", "f32"), (0, "f32"), (0, "bf16"), (0, "fp8")])
def test_scores_equal_the_padded_submit(fr, gpu, kind, prec):
    """fp32 on the mixed-width spec model and on shrunk Model-A; bf16 and fp8 on shrunk Model-A, as tests/test_gpu_pooled_modes.py does: the mixed
    model's record of 152 floats is no multiple of 16, and the library gives such a model no low-precision chain at all."""
    PC.check_scores(fr, gpu, kind, precision={"f32": None, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[prec])


def test_order_against_update_rows(fr, gpu):
    PC.check_order_against_update_rows(fr, gpu)


@pytest.mark.parametrize("pool", ["sum", "mean", "weighted"])
def test_server_answers_offsets_form_blocks_on_the_gpu(fr, gpu, pool):
    PC.check_server(fr, gpu, pool, free_port_block)


def test_server_ends_the_connection_on_a_bad_block(fr, gpu):
    PC.check_server_refuses_bad_block(fr, gpu, free_port_block, "nnz")


# the other instantiations: 4 items per thread (two half passes of 2), 2 items under weights and under MEAN -- odd batches, the last item's bag
MALFORMED_MORE = [("csr-4-2-false-wide-table", "sum", 37), ("csr-2-8-false-wide-bank", "weighted", 37), ("csr-2-2-false-mixed-bank", "mean", 3),
                  ("csr-1-16-false-wide-table", "sum", 37)]


@pytest.mark.parametrize("what", PC.MALFORMED)
@pytest.mark.parametrize("case_id,kind,B", MALFORMED_MORE)
def test_malformed_bag_on_the_other_instantiations(fr, gpu, case_id, kind, B, what):
    PC.check_malformed(fr, gpu, what, "last", kind=kind, case_id=case_id, B=B)

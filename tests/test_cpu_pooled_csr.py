"""The offsets (CSR) input form of the pooled lookups (include/fleetrec_serving.h: fr_worker_gather_pooled_csr, fr_worker_submit_pooled_csr_device,
fr_worker_submit_pooled_csr) on the CPU back-end (device = -1, csrc/fr_cpu.cpp frc_gather_pooled).  Runs without a GPU;
tests/test_gpu_pooled_csr.py runs the same checks (tests/pooled_csr.py) on the MI355X.

Bars: the offsets form's records equal, bit for bit and in every word, the numpy fold of the same bags AND the padded entry point's records on
the same context; scores equal the padded submit's bit for bit; a malformed bag is FR_ERR_INDEX_RANGE with every other bag's words intact."""
import pytest
from conftest import free_port_block

import pooled_csr as PC

CPU = -1
MODES = {"table": 0, "item": 1, "bank": 2}
CASE_KINDS = [(c, k) for c in PC.CASE_IDS for k in PC.KINDS]   # case-major: a case's inputs are built once for its three folds


@pytest.mark.parametrize("case_id,kind", CASE_KINDS)
def test_csr_case(fr, case_id, kind):
    PC.run_case(fr, CPU, case_id, kind)


@pytest.mark.parametrize("kind", PC.KINDS)
def test_caps_that_are_multiples_of_four(fr, kind):
    PC.run_case(fr, CPU, PC.CASE_CAPS4["id"], kind)


@pytest.mark.parametrize("case_id", [c for c in PC.CASE_IDS if "-mixed-" in c])
def test_arrays_off_a_16_byte_boundary(fr, case_id):
    """One case per window, weighted (all three arrays): offsets, indices and weights 4, 8 and 12 bytes past a 16-byte boundary in turn."""
    PC.run_case(fr, CPU, case_id, "weighted", shifts=((4, 8, 12), (8, 12, 4), (12, 4, 8)), batches=(3, 37))


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_cap_one_bags_of_one_equal_gather_only(fr, kind, mode):
    PC.check_cap1_is_gather_only(fr, CPU, kind, MODES[mode])


@pytest.mark.parametrize("place", ["first", "last"])
@pytest.mark.parametrize("what", PC.MALFORMED)
def test_malformed_bag(fr, what, place):
    PC.check_malformed(fr, CPU, what, place)


@pytest.mark.parametrize("what", PC.MALFORMED)
def test_malformed_bag_under_weights(fr, what):
    PC.check_malformed(fr, CPU, what, "last", kind="weighted")


@pytest.mark.parametrize("kind,mode", [(0, "table"), ("spec", "bank")])
def test_errors(fr, kind, mode):
    PC.check_errors(fr, CPU, kind, MODES[mode])


def test_sharded_contexts_refuse_the_offsets_form(fr):
    PC.check_sharded_refuses(fr, CPU)


@pytest.mark.parametrize("kind", ["spec", 0])
def test_scores_equal_the_padded_submit(fr, kind):
    PC.check_scores(fr, CPU, kind)


def test_order_against_update_rows(fr):
    PC.check_order_against_update_rows(fr, CPU)


@pytest.mark.parametrize("pool", ["sum", "mean", "weighted"])
def test_server_answers_offsets_form_blocks_on_the_cpu_back_end(fr, pool):
    PC.check_server(fr, CPU, pool, free_port_block)


@pytest.mark.parametrize("which", ["nnz", "first"])
def test_server_ends_the_connection_on_a_bad_block(fr, which):
    PC.check_server_refuses_bad_block(fr, CPU, free_port_block, which)


def test_hosts_refuse_csr_without_hots_and_with_stream_or_shards(fr):
    PC.check_hosts_csr_needs_hots(fr)


# the other instantiations: 4 items per thread (two half passes of 2), 2 items under weights and under MEAN -- odd batches, the last item's bag
MALFORMED_MORE = [("csr-4-2-false-wide-table", "sum", 37), ("csr-2-8-false-wide-bank", "weighted", 37), ("csr-2-2-false-mixed-bank", "mean", 3),
                  ("csr-1-16-false-wide-table", "sum", 37)]


@pytest.mark.parametrize("what", PC.MALFORMED)
@pytest.mark.parametrize("case_id,kind,B", MALFORMED_MORE)
def test_malformed_bag_on_the_other_instantiations(fr, case_id, kind, B, what):
    PC.check_malformed(fr, CPU, what, "last", kind=kind, case_id=case_id, B=B)

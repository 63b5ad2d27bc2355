"""Streaming pushes of pooled lookups (fr_worker_push_pooled_device, fr_worker_push_pooled_csr_device, fr_worker_push_pooled_device_list) on the
CPU back-end (device = -1: a push computes before it returns), and the accounting of libfleetrec.so's kernels.  Runs without a GPU;
tests/test_gpu_pooled_stream.py runs the same checks (tests/pooled_stream.py) and the operand's bytes on the MI355X.  No tolerance but the
1e-5 relative of include/fleetrec.h between the stage pipeline's and the fused kernel's one-hot sums.
Not here: the refusal while host-fed batches are queued in a block (pooled_stream.check_host_fed_block_refuses) -- the CPU back-end has no host-fed
streaming at all (fr_worker_push_host / fr_worker_stage_acquire are FR_ERR_STATE there), so a CPU worker can never hold a queued block; the case
below pins that, the GPU module runs the refusal itself."""
import os
import re

import pytest

import gather_matrix as GM
import pooled_stream as PS

CPU = -1


@pytest.mark.parametrize("kind,caps_kind", [("spec", "spread"), (0, "ones"), (2, "five")])
def test_pushed_scores_equal_the_submit_form(fr, kind, caps_kind):
    PS.check_scores_equal_submit(fr, CPU, kind, caps_kind=caps_kind)


@pytest.mark.parametrize("group", [8, None], ids=["group8", "default-group"])
def test_one_hot_and_pooled_pushes_alternate(fr, group):
    PS.check_mixing(fr, CPU, group)


def test_cpu_worker_cannot_queue_a_host_fed_block(fr):
    PS.check_cpu_has_no_host_fed_block(fr)


def test_update_rows_between_two_pooled_pushes(fr):
    PS.check_order_against_update_rows(fr, CPU)


def test_range_errors_among_clean_batches(fr):
    PS.check_range_errors(fr, CPU)


def test_state_and_arguments(fr):
    PS.check_state_and_arguments(fr, CPU)


def test_kernel_names_are_the_parents(fr):
    """The operand-store arms are arms of gather_pooled_kernel: libfleetrec.so holds the kernels it held before them, name for name
    (tests/golden/libfleetrec_kernel_names.txt: the list of the commit before the streaming pushes)."""
    from exact_chain import demangle
    names = sorted({demangle(r["name"]) for r in PS.kernel_records(fr)})
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "libfleetrec_kernel_names.txt")
    want = [ln.strip() for ln in open(golden) if ln.strip()]
    assert names == want, (sorted(set(names) - set(want)), sorted(set(want) - set(names)))


def test_pooled_shapes_keep_their_registers_with_the_operand_arms(fr):
    """tests/test_cpu_pooled_modes.py's bounds restated for this feature: all eight shapes of gather_pooled_kernel without a spilled register
    and without scratch, at most 64 VGPRs with 8 row words in flight per thread and at most 96 with 16."""
    from exact_chain import demangle
    shapes = set()
    for r in PS.kernel_records(fr):
        name = demangle(r["name"])
        if not name.startswith("gather_pooled_kernel"):
            continue
        items, win = re.match(r"gather_pooled_kernel<(\d+), (\d+), ", name).groups()
        shapes.add(name)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_count"] <= (64 if int(items) * int(win) <= 8 else 96), r
    assert shapes == set(GM.POOLED_HOTS), shapes

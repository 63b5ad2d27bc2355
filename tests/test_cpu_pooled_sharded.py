"""Multi-hot pooled lookups on table-sharded contexts, on the CPU back-end (device = -1): G CPU shard contexts of one process on the in-process
host exchange, fp32 throughout.  Runs without a GPU; tests/test_gpu_pooled_sharded.py runs the same checks (tests/pooled_sharded.py), the
low-precision slices and the fp8 calibration on the MI355X.  Also here, host only: the pre-check that the GPU cases' bags keep the bf16 / fp8
restatements of the chain inside their tolerances."""
import pytest

import pooled_sharded as PS

CPU = PS.CPU


@pytest.mark.parametrize("fold", ["sum", "mean", "weighted", "csr", "csr_weighted"])
def test_fp32_slices_equal_the_unsharded_records_columns(fr, fold):
    PS.check_fp32_slices(fr, CPU, (1, 2, 3, 8, 64), fold)


@pytest.mark.parametrize("G", [2, 3, 8])
def test_one_live_slot_per_bag_equals_one_hot(fr, G):
    PS.check_one_live_slot_equals_one_hot(fr, CPU, G, "f32")


@pytest.mark.parametrize("G,fold,B,csr", [(2, "sum", 301, True), (3, "mean", 301, False), (8, "weighted", 5, True)])
def test_real_bags_through_the_step(fr, G, fold, B, csr):
    PS.check_real_bags(fr, CPU, G, "f32", fold, B, csr)


@pytest.mark.parametrize("fold,B", [("sum", 301), ("mean", 301), ("weighted", 301), ("sum", 5)])
def test_chain_restatements_hold_on_the_gpu_cases_bags(fr, fold, B):
    PS.check_restatements_hold_on_the_chosen_bags(fr, 0, fold, B)   # (the GPU cases' row cap; nothing touches a device)


def test_errors_reach_the_owning_ranks(fr):
    PS.check_errors_reach_the_owning_ranks(fr, CPU)


def test_state_and_arguments(fr):
    PS.check_state_and_arguments(fr, CPU)

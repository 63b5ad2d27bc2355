"""Pooling modes (FR_POOL_SUM / FR_POOL_MEAN, fr_ctx_set_pooling_modes) and per-sample weights (fr_worker_*_pooled_weighted*,
include/fleetrec_serving.h) of the multi-hot lookups on the CPU back-end (device = -1, csrc/fr_cpu.cpp frc_gather_pooled).  Runs without a
GPU; tests/test_gpu_pooled_modes.py runs the same checks (tests/pooled_modes.py) on the MI355X.

Bars: records bit-exact against the contract folded in numpy (one np.float32 multiply, then sequential np.float32 adds; one np.float32
division by the bag's count) wherever the expectation is not a NaN, a NaN where it is; scores bit-exact against fr_worker_fc_only on the
expected records; the hosts' printed scores against an exact closed form.  No tolerance anywhere."""
import numpy as np
import pytest
from conftest import free_port_block

import gather_matrix as GM
import pooled_modes as PM

CPU = -1
MODES = {"table": 0, "item": 1, "bank": 2}   # fr.INDEX_PER_TABLE / PER_ITEM / PER_BANK
CASE_IDS = [c["id"] for c in GM.POOLED_CASES]


@pytest.mark.parametrize("what", ["weighted", "modes"])
@pytest.mark.parametrize("case_id", CASE_IDS)
def test_pooled_case(fr, case_id, what):
    """Checks 1 and 2 on every case of gather_matrix.POOLED_CASES (the case's inputs are built once for both)."""
    (PM.run_case_weighted if what == "weighted" else PM.run_case_modes)(fr, CPU, case_id)


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank")])
def test_all_ones_weights_equal_the_unweighted_records(fr, kind, mode):
    PM.check_ones_identity(fr, CPU, kind, MODES[mode])


@pytest.mark.parametrize("kind,mode", [(0, "table"), (2, "bank"), ("spec", "item")])
def test_one_slot_mean_equals_gather_only(fr, kind, mode):
    PM.check_hots1_mean_is_gather_only(fr, CPU, kind, MODES[mode])


@pytest.mark.parametrize("kind,mode", [(0, "table"), (1, "bank"), ("spec", "table")])
def test_even_odd_known_answers(fr, kind, mode):
    PM.check_even_odd_known_answers(fr, CPU, kind, MODES[mode])


@pytest.mark.parametrize("kind", ["spec", 0])
def test_scores_from_weighted_and_mean_records(fr, kind):
    PM.check_scores(fr, CPU, kind)


@pytest.mark.parametrize("kind,mode", [(0, "table"), ("spec", "bank")])
def test_errors(fr, kind, mode):
    PM.check_errors(fr, CPU, kind, MODES[mode])


def test_sharded_contexts_refuse_pooling_modes(fr):
    PM.check_sharded_refuses_modes(fr, CPU)


@pytest.mark.parametrize("pool,ragged", [("weighted", False), ("weighted", True), ("mean", False), ("mean", True)])
def test_server_answers_weighted_and_mean_requests_on_the_cpu_back_end(fr, pool, ragged):
    PM.check_server(fr, CPU, pool, ragged, free_port_block)


def test_hosts_refuse_pool_without_hots(fr):
    PM.check_server_pool_needs_hots(fr)


def test_pooled_kernels_have_no_spill_no_scratch_and_keep_their_occupancy(fr):
    """gather_pooled_kernel carries three arms (SUM, MEAN, weighted) and its register count is the largest arm's: the MEAN and weighted arms
    are shaped (half passes, weights a unit ahead of the fold) to stay inside the plain SUM fold's registers, and __launch_bounds__ holds every
    product shape at the waves per SIMD it had with the SUM fold alone.  Read from the code object's notes (tools/kernel_resources.py): all
    eight instantiations without a spilled register and without a scratch segment, at most 64 VGPRs (8 waves) with 8 row words in flight
    per thread, at most 96 (5 waves) with 16 -- a compiler that no longer manages this fails here, not on a user's GPU."""
    import importlib.util
    import os
    import re
    from exact_chain import demangle
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(root, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    recs = [r for r in kr.kernel_records(fr.LIB_PATH) if "gather_pooled_kernel" in r["name"]]
    shapes = set()
    for r in recs:
        name = demangle(r["name"])   # mangled or not, by the tool's c++filt
        items, win = re.match(r"gather_pooled_kernel<(\d+), (\d+), ", name).groups()
        shapes.add(name)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
        assert r["vgpr_count"] <= (64 if int(items) * int(win) <= 8 else 96), r
    assert shapes == set(GM.POOLED_HOTS), shapes

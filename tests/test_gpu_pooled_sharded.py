"""Multi-hot pooled lookups on table-sharded contexts, on the MI355X: G GPU shard contexts of one device on the staged exchange.  The checks are
tests/pooled_sharded.py's (tests/test_cpu_pooled_sharded.py runs the fp32 ones on the CPU back-end); here also the low-precision slices through
every shape the launcher can pick for them, the pooled fp8 calibration and the failure protocol.  Every case runs once."""
import pytest

import gather_matrix as GM
import pooled_sharded as PS

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kernel", list(GM.POOLED_HOTS), ids=[k[len("gather_pooled_kernel<"):-1].replace(", ", "-") for k in GM.POOLED_HOTS])
def test_fp32_slices_through_every_shape(fr, gpu, kernel):
    PS.check_fp32_slices(fr, gpu, GM.POOLED_HOTS[kernel], "sum", kernel)


@pytest.mark.parametrize("fold", ["mean", "weighted", "csr", "csr_weighted"])
def test_fp32_slices_of_every_fold(fr, gpu, fold):
    PS.check_fp32_slices(fr, gpu, (1, 2, 3, 8, 64), fold)


# every shape a bf16 / e4m3 slice can take: the six with the store arms, and the neighbours of the two without (longest bags of 1 and of 5)
@pytest.mark.parametrize("pattern", [(1,), (1, 2, 3), (1, 3, 5), (4,), (1, 2, 5, 8, 9, 15), (4, 8, 12), (1, 16, 17, 33, 63, 64), (4, 16, 20, 64)],
                         ids=lambda p: "-".join(str(h) for h in p))
def test_low_precision_slices_through_every_shape(fr, gpu, pattern):
    PS.check_lp_slices(fr, gpu, pattern)


@pytest.mark.parametrize("pattern,fold,shift", [((1, 3, 5), "mean", 0), ((4, 8, 12), "weighted", 0), ((1, 2, 5, 8, 9, 15), "csr", 0), ((1,), "csr_weighted", 0),
                                                ((4, 8, 12), "sum", 4), ((4, 16, 20, 64), "weighted", 8)])
def test_low_precision_slices_of_every_fold_and_unaligned_rows(fr, gpu, pattern, fold, shift):
    PS.check_lp_slices(fr, gpu, pattern, fold, shift, e_shift=2)


@pytest.mark.parametrize("G,prec", [(2, "f32"), (3, "bf16"), (8, "fp8"), (8, "f32")])
def test_one_live_slot_per_bag_equals_one_hot(fr, gpu, G, prec):
    PS.check_one_live_slot_equals_one_hot(fr, gpu, G, prec)


@pytest.mark.parametrize("G,prec,fold,B,csr", [(2, "f32", "sum", 301, True), (3, "bf16", "sum", 301, False), (8, "fp8", "sum", 301, True), (8, "f32", "weighted", 5, False),
                                              (3, "bf16", "mean", 301, True), (2, "fp8", "weighted", 301, False)])
def test_real_bags_through_the_step(fr, gpu, G, prec, fold, B, csr):
    PS.check_real_bags(fr, gpu, G, prec, fold, B, csr)


def test_calibration_sees_the_bags(fr, gpu):
    PS.check_calibration_sees_the_bags(fr, gpu)


def test_errors_reach_the_owning_ranks(fr, gpu):
    PS.check_errors_reach_the_owning_ranks(fr, gpu)


def test_state_and_arguments(fr, gpu):
    PS.check_state_and_arguments(fr, gpu)


def test_fc_failure_under_the_pooled_step_reaches_every_rank(fr, gpu):
    PS.check_fc_failure_reaches_every_rank(fr, gpu)

"""GPU parity of the table-sharded FC path on integer-valued data (tests/exact_sharded.py): G shard contexts on one device, every shard loaded
by upload alone, every comparison np.array_equal against the host's restatement of the chain -- slices in fp32 and in the transport types,
fr_worker_fc_from_slices[_lp] in the all-gather and the all-to-all layout, the fp8 calibration on slices and through the communicator, and the
whole fr_worker_submit_sharded step through the staged exchange in both exchange modes.  One test per (row, precision) of exact_sharded.ROWS."""
import pytest

import exact_sharded as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("r,prec", S.CELLS, ids=S.CELL_IDS)
def test_exact_sharded_row(fr, gpu, r, prec):
    S.check_row(fr, gpu, r, prec)


def test_bf16_refuses_a_record_that_is_no_multiple_of_16(fr, gpu):
    """Row e's K = 4200: the bf16 chain is refused on a shard context as on an unsharded one, and the context stays in fp32."""
    r = S.row("e")
    assert r["refused"] == ("bf16",)
    m = S.model_data(fr, r["model"])[0]
    assert m.record_len % 16 == 8
    c = fr.Context(m, device=gpu, shard_rank=1, n_shards=r["G"])
    try:
        with pytest.raises(fr.FleetRecError) as e:
            c.set_fc_precision(fr.FC_BF16)
        assert e.value.status == fr.FR_ERR_INVALID
    finally:
        c.close()


def test_dense_only_shard_loads_by_upload(fr, gpu):
    S.check_dense_only_shard_loads_by_upload(fr, gpu)


@pytest.mark.parametrize("prec", ["f32", "bf16", "fp8"])
def test_nan_table_value_reaches_exactly_its_two_items(fr, gpu, prec):
    S.check_nan_table_value(fr, gpu, prec)


def test_fp8_calibration_on_slices_ignores_stale_padding(fr, gpu):
    S.check_fp8_calibration_ignores_stale_padding(fr, gpu)

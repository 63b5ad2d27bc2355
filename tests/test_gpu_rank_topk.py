"""Segmented top-K ranking on the MI355X: the checks of tests/rank_topk.py on the device (the kernels of the companion code object,
libfleetrec_rank.so), and the host form's results against the CPU back-end's, bit for bit."""
import numpy as np
import pytest
from conftest import free_port_block

import rank_topk as R

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cls", R.CLASSES)
def test_values(fr, gpu, cls):
    R.check_values(fr, gpu, cls)


def test_segments(fr, gpu):
    R.check_segments(fr, gpu)


def test_long_segment(fr, gpu):
    R.check_long_segment(fr, gpu)


def test_malformed_offsets(fr, gpu):
    """(The bounds handling this exercises is safe by construction -- every load is behind the segment's own check -- and the CPU twin of the same
    cases runs under ASan + UBSan: make -C csrc san-rank-topk.)"""
    R.check_malformed(fr, gpu)


@pytest.mark.parametrize("group", [64, 1])
def test_stream_order(fr, gpu, group):
    R.check_stream_order(fr, gpu, group)


def test_host_form_equals_the_cpu_back_end(fr, gpu):
    on_gpu, on_cpu = R.host_form_results(fr, gpu), R.host_form_results(fr, R.CPU)
    assert [w for w, _, _ in on_gpu] == [w for w, _, _ in on_cpu]
    for (what, sg, (gi, gs)), (_, sc, (ci, cs)) in zip(on_gpu, on_cpu):
        if np.array_equal(sg, sc):   # the fp32 chain's scores of the two back-ends: where they agree bit for bit, so must the rankings
            assert np.array_equal(gi, ci) and np.array_equal(gs, cs), what
    # the rankings themselves on identical scores: the device form on both back-ends over the same bit patterns
    rng = np.random.default_rng(5900)
    bits = R.values("random_bits", 20000, rng)
    off = np.array([0, 1, 300, 300, 17000, 20000])
    got = []
    for device in (gpu, R.CPU):
        m, ctx = R.small_context(fr, device, 200)
        try:
            wk = fr.Worker(ctx, 16)
            got.append(R.rank(fr, ctx, wk, bits, 100, off))
            wk.close()
        finally:
            ctx.close()
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])


def test_errors(fr, gpu):
    R.check_errors(fr, gpu)


def test_server_topk_reply(fr, gpu):
    R.check_server(fr, gpu, free_port_block)

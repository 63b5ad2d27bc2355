"""Request-form batches on the MI355X: the checks of tests/request_form.py on the device (request_expand_kernel of the companion code object,
libfleetrec_request.so), the low-precision chains behind the expansion, and the results against the CPU back-end's."""
import numpy as np
import pytest
from conftest import free_port_block

import request_form as Q

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", Q.WORD_CASES)
def test_words(fr, gpu, case):
    Q.check_words(fr, gpu, case)


def test_segments(fr, gpu):
    Q.check_segments(fr, gpu)


def test_malformed_offsets(fr, gpu):
    """(The bounds handling this exercises is safe by construction -- the owner is clamped, every descriptor is inside its row -- and the CPU twin of
    the same cases runs under ASan + UBSan: make -C csrc san-request-expand.)"""
    Q.check_malformed(fr, gpu)


@pytest.mark.parametrize("kind,precision", [("A", "FC_FP32"), ("C", "FC_FP32"), ("C_bank", "FC_FP32"), ("narrow", "FC_FP32"), ("A", "FC_BF16"), ("C_bank", "FC_BF16"),
                                            ("C", "FC_FP8"), ("C_bank", "FC_FP8")])
def test_equality_through_the_existing_paths(fr, gpu, kind, precision):
    Q.check_equality(fr, gpu, kind, getattr(fr, precision))


@pytest.mark.parametrize("group", [64, 1])
def test_stream_order(fr, gpu, group):
    Q.check_stream_order(fr, gpu, group)


def test_host_form_equals_the_cpu_back_end(fr, gpu):
    on_gpu, on_cpu = Q.host_form_results(fr, gpu), Q.host_form_results(fr, Q.CPU)
    assert [w for w, _, _ in on_gpu] == [w for w, _, _ in on_cpu]
    for (what, sg, (gi, gs)), (_, sc, (ci, cs)) in zip(on_gpu, on_cpu):
        if np.array_equal(sg, sc):   # the fp32 chain's scores of the two back-ends: where they agree bit for bit, so must the rankings
            assert np.array_equal(gi, ci) and np.array_equal(gs, cs), what
    # the expanded rows themselves are identical on both back-ends, unconditionally
    for g, c in zip(Q.expanded_rows(fr, gpu), Q.expanded_rows(fr, Q.CPU)):
        assert np.array_equal(g, c)


def test_errors_and_state(fr, gpu):
    Q.check_errors(fr, gpu)


def test_server_request_form(fr, gpu):
    Q.check_server(fr, gpu, free_port_block)

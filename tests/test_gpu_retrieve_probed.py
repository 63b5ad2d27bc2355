"""Probed (IVF) retrieval on the MI355X: the checks of tests/retrieve_probed.py on the device (probe_sort_kernel, the two grouping kernels,
retrieve_probe_scan_kernel + the ranking companion + retrieve_rows_kernel), and the device's rows and score bits against the CPU back-end's on the
exact cases."""
import numpy as np
import pytest

import retrieve_probed as P

pytestmark = pytest.mark.gpu


def same(got, cpu):
    assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1]), "the device and the CPU back-end differ"


@pytest.mark.parametrize("dim,k,n_q,n_probe,kind", P.EXACT)
def test_exact(fr, gpu, dim, k, n_q, n_probe, kind):
    same(P.exact_case(fr, gpu, dim, k, n_q, n_probe, kind), P.exact_case(fr, P.CPU, dim, k, n_q, n_probe, kind))


@pytest.mark.parametrize("k", [64, 256])
def test_ties_across_lists(fr, gpu, k):
    same(P.ties_case(fr, gpu, k), P.ties_case(fr, P.CPU, k))


@pytest.mark.parametrize("dim,k", P.ADVERSARIAL)
def test_adversarial_order(fr, gpu, dim, k):
    same(P.adversarial_case(fr, gpu, dim, k), P.adversarial_case(fr, P.CPU, dim, k))


@pytest.mark.parametrize("dim", [32, 128])
def test_rounded_against_the_exact_call(fr, gpu, dim):
    P.check_rounded(fr, gpu, dim)


def test_composition_and_stream_order(fr, gpu):
    P.check_composition(fr, gpu)


def test_special_values(fr, gpu):
    P.check_special(fr, gpu)


def test_id_out_of_range(fr, gpu):
    P.check_index_range(fr, gpu)


@pytest.mark.parametrize("name", list(P.REFUSALS))
def test_refusals(fr, gpu, name):
    P.check_refusal(fr, gpu, name)

"""bf16 retrieval over a table image on the MI355X: the checks of tests/retrieve_lp.py on the device (retrieve_lp_image_kernel, retrieve_lp_scan_kernel +
the ranking companion + retrieve_rows_kernel), and the device's rows and score bits against the CPU back-end's on the exact cases."""
import numpy as np
import pytest

import retrieve_lp as T

pytestmark = pytest.mark.gpu


def same(got, cpu):
    assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1]), "the device and the CPU back-end differ"


@pytest.mark.parametrize("dim,n_q,k,n_rows,row0", T.EXACT)
def test_exact(fr, gpu, dim, n_q, k, n_rows, row0):
    same(T.exact_case(fr, gpu, dim, n_q, k, n_rows, row0), T.exact_case(fr, T.CPU, dim, n_q, k, n_rows, row0))


@pytest.mark.parametrize("dim,k", T.ADVERSARIAL)
def test_adversarial_order(fr, gpu, dim, k):
    same(T.adversarial_case(fr, gpu, dim, k), T.adversarial_case(fr, T.CPU, dim, k))


def test_special_values(fr, gpu):
    T.check_special(fr, gpu)


@pytest.mark.parametrize("dim", [32, 128])
def test_rounded(fr, gpu, dim):
    T.check_rounded(fr, gpu, dim)


def test_patch_equals_rebuild(fr, gpu):
    T.check_patch(fr, gpu)


@pytest.mark.parametrize("name", list(T.REFUSALS))
def test_refusals(fr, gpu, name):
    T.check_refusal(fr, gpu, name)

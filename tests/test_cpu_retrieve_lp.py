"""bf16 retrieval over a table image on the CPU back-end (device = -1): the checks of tests/retrieve_lp.py against the CPU twin (frc_retrieve_image), and
the companion code object's properties, which need no device."""
import pytest

import retrieve_lp as T

CPU = T.CPU


@pytest.mark.parametrize("dim,n_q,k,n_rows,row0", T.EXACT)
def test_exact(fr, dim, n_q, k, n_rows, row0):
    T.exact_case(fr, CPU, dim, n_q, k, n_rows, row0)


@pytest.mark.parametrize("dim,k", T.ADVERSARIAL)
def test_adversarial_order(fr, dim, k):
    T.adversarial_case(fr, CPU, dim, k)


def test_special_values(fr):
    T.check_special(fr, CPU)


@pytest.mark.parametrize("dim", [32, 128])
def test_rounded(fr, dim):
    T.check_rounded(fr, CPU, dim)


def test_patch_equals_rebuild(fr):
    T.check_patch(fr, CPU)


@pytest.mark.parametrize("name", list(T.REFUSALS))
def test_refusals(fr, name):
    T.check_refusal(fr, CPU, name)


def test_companion_code_object(fr):
    T.check_companion(fr)

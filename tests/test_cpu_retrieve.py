"""Top-K inner-product retrieval on the CPU back-end (device = -1): the checks of tests/retrieve.py against the CPU twin (frc_retrieve), and the
companion code object's properties, which need no device."""
import pytest

import retrieve as T

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


def test_stream_order(fr):
    T.check_stream_order(fr, CPU)


@pytest.mark.parametrize("name", [n for n in T.REFUSALS if "queued" not in n])   # (the CPU back-end computes a host-fed batch inside the push)
def test_refusals(fr, name):
    T.check_refusal(fr, CPU, name)


def test_companion_code_object(fr):
    T.check_companion(fr)

"""Probed (IVF) retrieval on the CPU back-end (device = -1): the checks of tests/retrieve_probed.py against the CPU twin (frc_retrieve_probed), and the
companion code object's properties, which need no device."""
import pytest

import retrieve_probed as P

CPU = P.CPU


@pytest.mark.parametrize("dim,k,n_q,n_probe,kind", P.EXACT)
def test_exact(fr, dim, k, n_q, n_probe, kind):
    P.exact_case(fr, CPU, dim, k, n_q, n_probe, kind)


@pytest.mark.parametrize("k", [64, 256])
def test_ties_across_lists(fr, k):
    P.ties_case(fr, CPU, k)


@pytest.mark.parametrize("dim,k", P.ADVERSARIAL)
def test_adversarial_order(fr, dim, k):
    P.adversarial_case(fr, CPU, dim, k)


@pytest.mark.parametrize("dim", [32, 128])
def test_rounded_against_the_exact_call(fr, dim):
    P.check_rounded(fr, CPU, dim)


def test_composition_and_stream_order(fr):
    P.check_composition(fr, CPU)


def test_special_values(fr):
    P.check_special(fr, CPU)


def test_id_out_of_range(fr):
    P.check_index_range(fr, CPU)


@pytest.mark.parametrize("name", list(P.REFUSALS))
def test_refusals(fr, name):
    P.check_refusal(fr, CPU, name)


def test_companion_code_object(fr):
    P.check_companion(fr)

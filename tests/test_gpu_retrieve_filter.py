"""Filtered bf16 retrieval on the MI355X: the checks of tests/retrieve_filter.py on the device (retrieve_filter_mask_kernel, retrieve_filter_scan_kernel,
retrieve_filter_merge_kernel), and the device's rows and score bits against the CPU back-end's."""
import numpy as np
import pytest

import retrieve_filter as T

pytestmark = pytest.mark.gpu


def same(got, cpu):
    assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1]), "the device and the CPU back-end differ"


@pytest.mark.parametrize("dim,n_q,k,row0", T.MASK)
def test_mask_at_tile_edges(fr, gpu, dim, n_q, k, row0):
    same(T.mask_case(fr, gpu, dim, n_q, k, row0), T.mask_case(fr, T.CPU, dim, n_q, k, row0))


@pytest.mark.parametrize("k,live", T.MERGE)
def test_short_and_empty_chunks(fr, gpu, k, live):
    same(T.merge_case(fr, gpu, k, live), T.merge_case(fr, T.CPU, k, live))


def test_two_level_merge(fr, gpu):
    same(T.long_case(fr, gpu), T.long_case(fr, T.CPU))


@pytest.mark.parametrize("n_excl", [1, 64])
def test_exclusions(fr, gpu, n_excl):
    same(T.exclude_case(fr, gpu, n_excl), T.exclude_case(fr, T.CPU, n_excl))


def test_adversarial_order_with_exclusions(fr, gpu):
    same(T.adversarial_case(fr, gpu), T.adversarial_case(fr, T.CPU))


def test_equivalence_and_stream_order(fr, gpu):
    T.check_equivalence_and_stream_order(fr, gpu)


@pytest.mark.parametrize("name", list(T.REFUSALS))
def test_refusals(fr, gpu, name):
    T.check_refusal(fr, gpu, name)


def test_filter_refusals(fr, gpu):
    T.check_filter_refusals(fr, gpu)

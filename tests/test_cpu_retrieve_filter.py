"""Filtered bf16 retrieval on the CPU back-end (device = -1): the checks of tests/retrieve_filter.py against the CPU twin (frc_retrieve_image_filtered), and
the companion code object's properties, which need no device."""
import pytest

import retrieve_filter as T

CPU = T.CPU


@pytest.mark.parametrize("dim,n_q,k,row0", T.MASK)
def test_mask_at_tile_edges(fr, dim, n_q, k, row0):
    T.mask_case(fr, CPU, dim, n_q, k, row0)


@pytest.mark.parametrize("k,live", T.MERGE)
def test_short_and_empty_chunks(fr, k, live):
    T.merge_case(fr, CPU, k, live)


def test_two_level_merge(fr):
    T.long_case(fr, CPU)


@pytest.mark.parametrize("n_excl", [1, 64])
def test_exclusions(fr, n_excl):
    T.exclude_case(fr, CPU, n_excl)


def test_adversarial_order_with_exclusions(fr):
    T.adversarial_case(fr, CPU)


def test_equivalence_and_stream_order(fr):
    T.check_equivalence_and_stream_order(fr, CPU)


@pytest.mark.parametrize("name", list(T.REFUSALS))
def test_refusals(fr, name):
    T.check_refusal(fr, CPU, name)


def test_filter_refusals(fr):
    T.check_filter_refusals(fr, CPU)


def test_companion_code_object(fr):
    T.check_companion(fr)

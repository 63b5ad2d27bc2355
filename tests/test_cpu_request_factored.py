"""Factored request-form batches on the CPU back-end (frc_reqfc, fr_cpu.cpp): the checks of tests/request_factored.py on device = -1."""
import pytest

import request_factored as F


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "bias+relu"])
@pytest.mark.parametrize("shape", list(F.SHAPES))
def test_exact_scores(fr, shape, epi):
    F.check_shape(fr, F.CPU, "f32", epi, shape)


def test_malformed_offsets(fr):
    F.check_malformed(fr, F.CPU)


@pytest.mark.parametrize("which", [r for r in F.REFUSALS if r != "fp8"])   # (the CPU back-end has no fp8 chain to refuse)
def test_refusals(fr, which):
    F.check_refusal(fr, F.CPU, which)

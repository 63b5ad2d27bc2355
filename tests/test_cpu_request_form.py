"""Request-form batches on the CPU back-end (device = -1): the checks of tests/request_form.py against the CPU twin (frc_expand_requests), and the
request companion code object's properties, which need no device."""
import pytest
from conftest import free_port_block

import request_form as Q

CPU = Q.CPU


@pytest.mark.parametrize("case", Q.WORD_CASES)
def test_words(fr, case):
    Q.check_words(fr, CPU, case)


def test_segments(fr):
    Q.check_segments(fr, CPU)


def test_malformed_offsets(fr):
    Q.check_malformed(fr, CPU)


@pytest.mark.parametrize("kind", ["A", "C", "C_bank", "narrow"])
def test_equality_through_the_existing_paths(fr, kind):
    Q.check_equality(fr, CPU, kind)


@pytest.mark.parametrize("group", [64, 1])
def test_stream_order(fr, group):
    Q.check_stream_order(fr, CPU, group)


def test_host_form(fr):
    Q.host_form_results(fr, CPU)


def test_errors_and_state(fr):
    Q.check_errors(fr, CPU)


def test_server_request_form(fr):
    Q.check_server(fr, CPU, free_port_block)


def test_companion_code_object(fr):
    Q.check_companion(fr)

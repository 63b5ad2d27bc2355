"""Segmented top-K ranking on the CPU back-end (device = -1): the checks of tests/rank_topk.py against the CPU twin (frc_rank_topk), and the
companion code object's properties, which need no device."""
import pytest
from conftest import free_port_block

import rank_topk as R

CPU = R.CPU


@pytest.mark.parametrize("cls", R.CLASSES)
def test_values(fr, cls):
    R.check_values(fr, CPU, cls)


def test_segments(fr):
    R.check_segments(fr, CPU)


def test_long_segment(fr):
    R.check_long_segment(fr, CPU)


def test_malformed_offsets(fr):
    R.check_malformed(fr, CPU)


@pytest.mark.parametrize("group", [64, 1])
def test_stream_order(fr, group):
    R.check_stream_order(fr, CPU, group)


def test_host_form(fr):
    R.host_form_results(fr, CPU)


def test_errors(fr):
    R.check_errors(fr, CPU)


def test_server_topk_reply(fr):
    R.check_server(fr, CPU, free_port_block)


def test_companion_code_object(fr):
    R.check_companion(fr)

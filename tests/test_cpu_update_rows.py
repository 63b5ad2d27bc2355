"""Sparse row updates on the CPU back-end (device = -1): the checks of tests/update_rows.py that need no GPU -- addressing in the plain and the
bank-interleaved layout with its tail, range and arguments, duplicates, the order on one worker, fleetrec_server --update-port.  (The same host code runs under
AddressSanitizer + UBSan in a program of its own: tools/update_rows_san.cpp, `make -C csrc san-update-rows`.)"""
import pytest
from conftest import free_port_block

import update_rows as U


@pytest.mark.parametrize("form", U.FORMS)
@pytest.mark.parametrize("mode", ["bank", "table"])
def test_addressing(fr, mode, form):
    U.check_addressing(fr, U.CPU, mode, form)


def test_range_and_arguments(fr):
    U.check_range_and_arguments(fr, U.CPU)


def test_duplicates(fr):
    U.check_duplicates(fr, U.CPU)


@pytest.mark.parametrize("group", [64, 1])
def test_order_on_one_worker(fr, group):
    U.check_order_on_one_worker(fr, U.CPU, group)


def test_server_update_port(fr):
    U.check_server(fr, U.CPU, free_port_block)


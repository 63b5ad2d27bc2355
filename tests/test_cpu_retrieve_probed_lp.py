"""Probed bf16 retrieval over the table image on the CPU back-end (device = -1): the checks of tests/retrieve_probed_lp.py against the CPU twin
(frc_retrieve_probed_image), and the companion code object's properties, which need no device."""
import pytest

import retrieve_probed_lp as PL


@pytest.mark.parametrize("name", list(PL.CHECKS))
def test_probed_image(fr, name):
    check, args = PL.CHECKS[name]
    check(fr, PL.CPU, *args)


def test_companion_code_object(fr):
    PL.check_companion(fr)

"""Probed bf16 retrieval over the table image on the MI355X: the checks of tests/retrieve_probed_lp.py on the device (the tenth companion's grouping
kernels, retrieve_probe_lp_scan_kernel + the ranking companion + retrieve_rows_kernel), and the device's rows and score bits against the CPU
back-end's wherever a check returns its result (the exact cases, the ties, the adversarial order)."""
import numpy as np
import pytest

import retrieve_probed_lp as PL

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(PL.CHECKS))
def test_probed_image(fr, gpu, name):
    check, args = PL.CHECKS[name]
    got = check(fr, gpu, *args)
    if got is not None:
        cpu = check(fr, PL.CPU, *args)
        assert np.array_equal(got[0], cpu[0]) and np.array_equal(got[1], cpu[1]), "the device and the CPU back-end differ"

"""Row pools on the MI355X: the checks of tests/key_admit.py on the device (keyadmit_admit_kernel, keyadmit_settle_kernel, keyadmit_release_kernel and
keyadmit_mark_kernel of the companion code object libfleetrec_admit.so), two workers admitting into one column with no sync between them, and the
tally of live bytes."""
import os
import subprocess
import sys

import pytest
from gpu_helpers import *  # noqa: F401,F403

import key_admit as KA

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("miss_kind", KA.MISS_KINDS)
def test_admit(fr, gpu, miss_kind):
    KA.check_admit(fr, gpu, miss_kind)


def test_idempotence_and_mixtures(fr, gpu):
    KA.check_mixture(fr, gpu)


@pytest.mark.parametrize("revive", [0, 1])
def test_duplicates(fr, gpu, revive):
    KA.check_duplicates(fr, gpu, revive)


@pytest.mark.parametrize("n_rows", KA.EXHAUST_POOLS)
def test_exhaustion(fr, gpu, n_rows):
    KA.check_exhaustion(fr, gpu, n_rows)


def test_map_full_before_the_pool(fr, gpu):
    KA.check_map_full(fr, gpu)


def test_erase_releases(fr, gpu):
    KA.check_erase_releases(fr, gpu)


def test_pool_over_an_existing_map(fr, gpu):
    KA.check_existing_map(fr, gpu)


def test_one_stream(fr, gpu):
    KA.check_one_stream(fr, gpu)


def test_two_workers_racing(fr, gpu):
    KA.check_two_workers(fr, gpu)


def test_arguments_and_state(fr, gpu):
    KA.check_arguments(fr, gpu)


def test_companion_code_object(fr, gpu):
    KA.check_companion(fr)


CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import __graft_entry__ as g
import key_admit
fr = g.load_package()

def live():
    out = (ctypes.c_uint64 * 2)()
    fr.lib().fr_exp_live_bytes(out)
    return out[0], out[1]

before = live()
for c in range(3):
    key_admit.lifetime_cycle(fr, %d, np.random.default_rng(c), live)
    print("cycle", c, "live bytes (device, pinned)", live(), "before", before, flush=True)
    assert live() == before, (c, live(), before)
print("ok")
"""


def test_lifetime_cycles_return_every_device_and_pinned_byte(fr, gpu):
    """Create / set pool / admit / erase / rebuild / set again / drop / destroy (key_admit.lifetime_cycle) in a child process on the experiments
    build, which exports the library's tally of live bytes: a same-size rebuild and a pool set again leave it where it was, and after every cycle it
    is exactly what it was before the first."""
    exp = os.path.join(os.path.dirname(fr.LIB_PATH), "libfleetrec_exp.so")
    if not os.path.exists(exp):
        pytest.skip("experiments library not built (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT, gpu)], env=dict(os.environ, FR_LIB=exp), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])

"""Keyed lookups on the MI355X: the checks of tests/keyed.py on the device (key_resolve_kernel, key_put_kernel, key_fill_kernel of the companion code
object libfleetrec_keys.so), the low-precision chains behind the resolve, the results against the CPU back-end's, and the tally of live bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
from gpu_helpers import *  # noqa: F401,F403

import keyed as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", K.WORD_CASES)
def test_words(fr, gpu, kind):
    K.check_words(fr, gpu, kind)


def test_probe_chains(fr, gpu):
    K.check_probe_chains(fr, gpu)


def test_puts(fr, gpu):
    K.check_puts(fr, gpu)


@pytest.mark.parametrize("kind,precision,pooled", [("A", "FC_FP32", 0), ("C_bank", "FC_BF16", 0), ("C", "FC_FP8", 0), ("narrow", "FC_FP32", 2)])
def test_equality_through_the_existing_paths(fr, gpu, kind, precision, pooled):
    K.check_equality(fr, gpu, kind, getattr(fr, precision), pooled)


def test_request_form(fr, gpu):
    K.check_request_form(fr, gpu)


def test_host_form_equals_the_cpu_back_end(fr, gpu):
    on_gpu, on_cpu = K.host_form_results(fr, gpu), K.host_form_results(fr, K.CPU)
    assert [w for w, _, _, _ in on_gpu] == [w for w, _, _, _ in on_cpu]
    for (what, rg, sg, (gi, gs)), (_, rc, sc, (ci, cs)) in zip(on_gpu, on_cpu):
        assert np.array_equal(rg, rc), what             # the resolved rows: unconditionally
        if np.array_equal(sg, sc):                      # the fp32 chain's scores of the two back-ends: where they agree bit for bit, so must the rankings
            assert np.array_equal(gi, ci) and np.array_equal(gs, cs), what


def test_misses(fr, gpu):
    K.check_misses(fr, gpu)


def test_errors_and_state(fr, gpu):
    K.check_errors(fr, gpu)


CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import __graft_entry__ as g
import keyed
fr = g.load_package()

def live():
    out = (ctypes.c_uint64 * 2)()
    fr.lib().fr_exp_live_bytes(out)
    return out[0], out[1]

m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=4096)
before = live()
for c in range(3):
    keyed.lifetime_cycle(fr, m, %d, np.random.default_rng(c))
    print("cycle", c, "live bytes (device, pinned)", live(), "before", before, flush=True)
    assert live() == before, (c, live(), before)
print("ok")
"""


def test_lifetime_cycles_return_every_device_and_pinned_byte(fr, gpu):
    """Key spaces set, replaced and dropped, workers and contexts coming and going (keyed.lifetime_cycle) in a child process on the experiments build,
    which exports the library's tally of live bytes: after every cycle it is exactly what it was before the first."""
    exp = os.path.join(os.path.dirname(fr.LIB_PATH), "libfleetrec_exp.so")
    if not os.path.exists(exp):
        pytest.skip("experiments library not built (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT, gpu)], env=dict(os.environ, FR_LIB=exp), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])

"""The life cycle of a key map on the MI355X: the checks of tests/key_lifecycle.py on the device (keymap_erase_kernel and keymap_walk_kernel of the
companion code object libfleetrec_keymaint.so), the results against the CPU back-end's, and the tally of live bytes."""
import os
import subprocess
import sys

import numpy as np
import pytest
from gpu_helpers import *  # noqa: F401,F403

import key_lifecycle as KL

pytestmark = pytest.mark.gpu


def same_as_cpu(on_gpu, on_cpu):
    assert [w for w, _, _, _ in on_gpu] == [w for w, _, _, _ in on_cpu]
    for (what, sg, eg, rg), (_, sc, ec, rc) in zip(on_gpu, on_cpu):
        assert sg == sc and eg == ec and rg == rc, what      # stats, sorted exports, resolved rows


def test_erase_and_export_and_the_cpu_back_end(fr, gpu):
    same_as_cpu(KL.check_erase(fr, gpu), KL.check_erase(fr, KL.CPU))


def test_export_of_an_empty_map_and_of_one_built_by_worker_puts(fr, gpu):
    KL.check_export_empty_and_device_built(fr, gpu)


def test_chains_and_the_cpu_back_end(fr, gpu):
    same_as_cpu(KL.check_chains(fr, gpu), KL.check_chains(fr, KL.CPU))


def test_stream_order(fr, gpu):
    KL.check_stream_order(fr, gpu, two_workers=True)


def test_rebuild_and_the_cpu_back_end(fr, gpu):
    same_as_cpu(KL.check_rebuild(fr, gpu), KL.check_rebuild(fr, KL.CPU))


def test_more_than_one_trip_of_the_walk(fr, gpu):
    KL.check_big_walk(fr, gpu)


@pytest.mark.parametrize("kind,pooled", [("A", 0), ("narrow", 2)])
def test_through_the_paths(fr, gpu, kind, pooled):
    KL.check_paths(fr, gpu, kind, pooled)


CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import __graft_entry__ as g
import key_lifecycle
fr = g.load_package()

def live():
    out = (ctypes.c_uint64 * 2)()
    fr.lib().fr_exp_live_bytes(out)
    return out[0], out[1]

m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=4096)
before = live()
for c in range(3):
    key_lifecycle.lifetime_cycle(fr, m, %d, np.random.default_rng(c), live)
    print("cycle", c, "live bytes (device, pinned)", live(), "before", before, flush=True)
    assert live() == before, (c, live(), before)
print("ok")
"""


def test_lifetime_cycles_return_every_device_and_pinned_byte(fr, gpu):
    """Rebuilds to larger / smaller / equal, exports and ctx-form erases (key_lifecycle.lifetime_cycle) in a child process on the experiments build,
    which exports the library's tally of live bytes: a same-size rebuild leaves it where it was, and after every cycle it is exactly what it was
    before the first."""
    exp = os.path.join(os.path.dirname(fr.LIB_PATH), "libfleetrec_exp.so")
    if not os.path.exists(exp):
        pytest.skip("experiments library not built (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT, gpu)], env=dict(os.environ, FR_LIB=exp), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])

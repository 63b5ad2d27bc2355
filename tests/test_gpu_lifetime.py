"""Who releases what (csrc/fr_mem.h) on the device: three create-use-destroy cycles of tests/lifetime.py that make every lazily allocated buffer
once -- the host ring with its events and copy stream, the batch-list ring, the bf16 / e4m3 weight copies and the reduction scratch, a per-bank
bf16 context, the pooled descriptors and the request split (each replaced once), the row-update staging (8, then 64 rows), the ranking's scratch
(16 385 scores) and host staging (3, then 9 segments), two shard contexts with a staged G = 2 step in each exchange mode, a worker closed after
its context -- and release everything with close() / free().  The library's own tally of live device and pinned bytes is then EXACTLY what it was
before the first cycle (the device's free memory, which other users of the machine change, is not looked at), and the fp32 scores of one fixed
batch are the same bits in the first and the last cycle.  The tally's reader (fr_exp_live_bytes) is exported by the experiments build only, so
the cycles run in a child process on that build, with FR_FUSED_HK=1: the persistent bf16 kernel then takes the 12-batch group, which is what
makes the batch-list ring."""
import os
import subprocess
import sys

import pytest
from gpu_helpers import *  # noqa: F401,F403

pytestmark = pytest.mark.gpu

CHILD = r"""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import __graft_entry__ as g
import lifetime
fr = g.load_package()

def live():
    out = (ctypes.c_uint64 * 2)()
    fr.lib().fr_exp_live_bytes(out)
    return out[0], out[1]

m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=4096)
rng = np.random.default_rng(3)
idx = lifetime.rows_of(rng, m, lifetime.B)
before = live()
scores = []
for c in range(3):
    scores.append(lifetime.cycle(fr, m, %d, idx, None))
    print("cycle", c, "live bytes (device, pinned)", live(), "before", before, flush=True)
    assert live() == before, (c, live(), before)
assert np.isfinite(scores[0]).all() and np.abs(scores[0]).max() > 0
assert np.array_equal(scores[0], scores[2]) and np.array_equal(scores[0], scores[1])
print("ok")
"""


def test_three_cycles_return_every_device_and_pinned_byte(fr, gpu):
    exp = os.path.join(os.path.dirname(fr.LIB_PATH), "libfleetrec_exp.so")
    if not os.path.exists(exp):
        pytest.skip("experiments library not built (make -C gpu-fpga-recommendation-system_amd/csrc exp)")
    env = dict(os.environ, FR_LIB=exp, FR_FUSED_HK="1")
    p = subprocess.run([sys.executable, "-c", CHILD % (ROOT, ROOT, gpu)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert p.returncode == 0 and b"ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])

"""Who releases what (csrc/fr_mem.h) on the CPU back-end: the create-use-destroy cycles of tests/lifetime.py through the Python binding on
device = -1 -- the scenarios of tools/lifetime_san.cpp -- leave the scores of a fixed batch bit-identical, and the sanitizer program itself
(ASan + UBSan host objects, the tally of live bytes, the leak checker at exit) runs clean."""
import os
import subprocess

import numpy as np

import lifetime
from conftest import ROOT


def test_cycles_leave_the_scores_of_a_fixed_batch_bit_identical(fr):
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=2048)   # (the one built-in model with dense features: dense_shared on and off)
    rng = np.random.default_rng(3)
    idx, dense = lifetime.rows_of(rng, m, lifetime.B), lifetime.dense_of(rng, m, lifetime.B)
    got = [lifetime.cycle(fr, m, -1, idx, dense) for _ in range(3)]
    assert np.isfinite(got[0]).all() and np.abs(got[0]).max() > 0
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_lifetime_sanitizer_program_runs_clean():
    p = subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "csrc"), "san-lifetime"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"lifetime_san: ok" in p.stdout, p.stdout[-3000:]

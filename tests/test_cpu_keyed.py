"""Keyed lookups on the CPU back-end (device = -1): the checks of tests/keyed.py against the CPU twins (frc_resolve_keys / frc_put_keys), the keys
companion code object's properties, which need no device, and the sanitizer program."""
import os
import subprocess

import numpy as np
import pytest

import keyed as K
import lifetime

CPU = K.CPU


@pytest.mark.parametrize("kind", K.WORD_CASES)
def test_words(fr, kind):
    K.check_words(fr, CPU, kind)


def test_probe_chains(fr):
    K.check_probe_chains(fr, CPU)


def test_puts(fr):
    K.check_puts(fr, CPU)


@pytest.mark.parametrize("kind,pooled", [("A", 0), ("C_bank", 0), ("C", 0), ("narrow", 2)])
def test_equality_through_the_existing_paths(fr, kind, pooled):
    K.check_equality(fr, CPU, kind, None, pooled)


def test_request_form(fr):
    K.check_request_form(fr, CPU)


def test_host_form(fr):
    K.host_form_results(fr, CPU)


def test_misses(fr):
    K.check_misses(fr, CPU)


def test_errors_and_state(fr):
    K.check_errors(fr, CPU)


def test_companion_code_object(fr):
    K.check_companion(fr)


def test_lifetime_cycles(fr):
    m = fr.Model.builtin(fr.MODEL_C).clone(max_rows=2048)
    for c in range(3):
        K.lifetime_cycle(fr, m, CPU, np.random.default_rng(c))


def test_keyed_sanitizer_program_runs_clean():
    p = subprocess.run(["make", "-s", "-j8", "-C", os.path.join(K.ROOT, "gpu-fpga-recommendation-system_amd", "csrc"), "san-keyed"],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=900)
    assert p.returncode == 0 and b"keyed_san: ok" in p.stdout, p.stdout[-3000:]

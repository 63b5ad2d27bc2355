"""What every companion code object (libfleetrec_rank / _request / _keys / _keymaint / _admit.so) must be, stated once: tests/rank_topk.py,
request_form.py, keyed.py, key_lifecycle.py and key_admit.py call check_companion with their library's launchers, kernels and marker."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def exported(lib_path):
    """the text symbols a shared library exports, sorted"""
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib_path]).decode()
    return sorted(l.split()[-1] for l in out.splitlines() if " T " in l)


def check_companion(fr, lib_path, launchers, kernel_counts, marker, other_libs, max_vgprs=64):
    """lib_path exists, imports neither getenv nor any fr_* / frc_* symbol, exports exactly `launchers`, and libfleetrec.so names it and $ORIGIN.
    With llvm-readelf (skipped, with the reason, without it): its kernels are exactly kernel_counts ({name part: instantiations}), none spills a
    register or has a private segment or needs more than max_vgprs VGPRs (None: no cap), and no kernel whose name holds `marker` sits in other_libs."""
    name = os.path.basename(lib_path)
    assert os.path.exists(lib_path), "the companion code object %s has not been built" % name
    und = subprocess.check_output(["nm", "-D", "--undefined-only", lib_path]).decode()
    assert "getenv" not in und, "%s imports getenv" % name
    assert not [l for l in und.splitlines() if l.split()[-1].startswith(("fr_", "frc_"))], "%s calls into the library" % name
    assert exported(lib_path) == sorted(launchers), exported(lib_path)
    need = subprocess.check_output(["readelf", "-d", fr.LIB_PATH]).decode()
    assert name in need and "$ORIGIN" in need, "libfleetrec.so does not link %s through $ORIGIN" % name
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not available: the kernel list and the register / scratch checks of %s did not run" % name)
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    recs = kr.kernel_records(lib_path)
    names = [r["name"] for r in recs]   # (mangled where llvm-cxxfilt is missing)
    assert {k: sum(k in n for n in names) for k in kernel_counts} == dict(kernel_counts) and len(names) == sum(kernel_counts.values()), names
    for r in recs:
        assert marker in r["name"], r["name"]
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r
        assert max_vgprs is None or r["vgpr_count"] <= max_vgprs, r                              # 64: eight waves per SIMD
    for other in other_libs:
        assert not [r["name"] for r in kr.kernel_records(other) if marker in r["name"]], "a %s kernel inside %s" % (marker, other)

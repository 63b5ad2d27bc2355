"""Register budget of the 64-item fp32 fused kernel, both compile forms (no GPU): fr_fused_tile_m2_kernel<44> of libfleetrec.so and
fr_epi_tile_m2_kernel<44> of libfleetrec_epi.so keep the late slice of their sliced gather in registers under FC1's first groups, beside
two FC1 accumulator pairs, the FC2 accumulators and the weight ring.  One workgroup per CU is two waves per SIMD: 256 registers per lane, and
a spill or a scratch segment would put vmcnt(0) waits into the straight-line MFMA segments.  Read from the code objects' metadata notes the way
tests/test_abi.py reads them (tools/kernel_resources.py)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _records(path):
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(ROOT, "tools", "kernel_resources.py"))
    kr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(kr)
    return kr.kernel_records(path)


@pytest.mark.parametrize("lib_name, kernel", [("libfleetrec.so", "fr_fused_tile_m2_kernel<44>"), ("libfleetrec_epi.so", "fr_epi_tile_m2_kernel<44>")])
def test_m2_kernels_fit_the_register_file_without_spills(fr, lib_name, kernel):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("llvm-readelf not available")
    path = os.path.join(os.path.dirname(fr.LIB_PATH), lib_name)
    base = kernel.split("<")[0]   # (the records name a kernel demangled where the demangler knows the ABI, else mangled: `...kernelILi44EE...`)
    recs = [r for r in _records(path) if base in r["name"] and ("<44>" in r["name"] or "ILi44EE" in r["name"])]
    assert len(recs) == 1, [r["name"] for r in _records(path) if "m2" in r["name"]]
    r = recs[0]
    assert r["vgpr_count"] <= 256, r
    assert r["vgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, r

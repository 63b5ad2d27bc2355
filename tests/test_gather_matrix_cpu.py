"""The gather matrix (tests/gather_matrix.py) on a machine without a GPU: its fp32 cases on the library's CPU back-end against the same
segment-by-segment reference (which pins that back-end and proves the reference and the case table before any GPU run), the premises of
the case table (every case's shape selects the kernel it names by the launchers' own rules; the bags hold every edge the pooled fold has),
the rounding helpers against torch's bfloat16 / float8_e4m3fn conversions on the exhaustive table, and completeness: every gather kernel
of libfleetrec.so is named by exactly the cases, every other kernel is an FC-chain kernel (tests/exact_chain.py) or listed in
COVERED_ELSEWHERE with the test that runs it."""
import os
import shutil
import sys

import numpy as np
import pytest

import exact_chain as E
import gather_matrix as G
import pooled_helpers as P
from gpu_helpers import ROOT, bf16_round, e4m3_encode

CPU_CASES = [c for c in G.CASES if c["tp"] == 0 and not c["big"]]


@pytest.mark.parametrize("case", CPU_CASES, ids=[c["id"] for c in CPU_CASES])
def test_onehot_case_on_the_cpu_back_end(fr, case):
    """Guarded destination, every batch, both out-of-range indices and the clean gather after each: as on the GPU."""
    G.run_onehot(fr, G.CPU, case, assert_kernel=False)


@pytest.mark.parametrize("case", G.POOLED_CASES, ids=[c["id"] for c in G.POOLED_CASES])
def test_pooled_case_on_the_cpu_back_end(fr, case):
    G.run_pooled(fr, G.CPU, case, assert_kernel=False)


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_onehot_case_selects_the_kernel_it_names(fr, case):
    """gather_launch's rules restated (onehot_kernel_for) on the case's own shape; index 0 and the last row in every column; what the case
    is there for (a partial last wave, a record past 200 MiB, pad columns, few / all-distinct rows for the item-tile kernels)."""
    m = G.make_model(fr, case["model"], case["mode"])
    offs, lens, F = m.shard_plan(case["shards"]) if case["shards"] > 1 else ([0], [m.record_len], m.record_len)
    for own in lens:
        for B in case["batches"]:
            assert G.onehot_kernel_for(own // 4, F // 4, B, case["tp"], case["variant"], bool(case["plan"])) == case["kernel"], (own, B)
    _, idx, _ = G.case_data(m, case)
    ranges = m.index_ranges()
    assert (idx[0] == 0).all() and (idx >= 0).all() and (idx < ranges[None, :]).all()
    if len(idx) > 1:
        assert (idx[1] == ranges - 1).all()
    if case["model"] == "narrow":
        assert (m.record_len // 4) % 64 and m.record_len // 4 > 64 and {t.dim for t in m.tables()} >= {4, 8, 16, 32, 64}
    if case["big"]:
        B = case["batches"][0]
        assert B * m.record_len * G.ESZ[case["tp"]] > 200 << 20 and (B - 3) * m.record_len * G.ESZ[case["tp"]] > 200 << 20 and B % 4 == 3
    if case["shards"] > 1:
        assert min(lens) < F and min(lens) // 4 >= 512
    if case["variant"] in ("tile", "dedup"):
        assert len(np.unique(idx[2:, 0])) <= 8 and any(len(np.unique(idx[2:, c])) == len(idx) - 2 for c in range(1, idx.shape[1]))


def test_the_matrix_covers_what_it_promises(fr):
    """Across the one-hot cases: every index mode, a dense block in the middle of a record, a COPY pad, a sharded context."""
    assert {c["mode"] for c in G.CASES} == {"table", "bank", "item"}
    for name in ("narrow", "wide"):
        m = G.make_model(fr, name)
        kinds = [s.kind for s in m.segments()]
        assert 0 < kinds.index(fr.SEG_DENSE) < len(kinds) - 1 and fr.SEG_COPY in kinds
    assert any(c["shards"] > 1 for c in G.CASES)
    assert G.make_model(fr, "noplan").record_len // 4 > 2048 and G.make_model(fr, "wide").record_len // 4 >= 512


@pytest.mark.parametrize("case", G.POOLED_CASES, ids=[c["id"] for c in G.POOLED_CASES])
def test_pooled_case_selects_the_kernel_it_names(fr, case):
    """frk_gather_pooled's rules restated (pooled_kernel_for); the bags hold an empty first slot, an empty last slot, only the last slot
    filled, whole empty bags, and special rows (-0.0, a signalling NaN, +-inf, a subnormal) only ever as a bag's lone non-empty slot."""
    m = G.make_model(fr, case["model"], case["mode"])
    tables, hots, idx, dense = G.pooled_data(m, case)
    assert G.pooled_kernel_for(hots) == case["kernel"]
    if case["kernel"].endswith("true>"):
        assert G.pooled_kernel_for(hots, aligned=False) == case["kernel"].replace("true>", "false>")
    pre = P.prefix_of(hots)
    seen = set()
    lone_special = 0
    for c, h in enumerate(hots):
        bag = idx[:, pre[c]:pre[c] + h]
        full = bag != -1
        special = np.isin(bag, list(G.SPECIAL_ROWS))
        assert not (special & (full.sum(axis=1) > 1)[:, None]).any()
        lone_special += int(special.any(axis=1).sum())
        assert (bag[full] >= 0).all() and (bag[full] < m.index_ranges()[c]).all()
        if (~full).all(axis=1).any():
            seen.add("empty bag")
        if h > 1:
            some = full.any(axis=1)
            seen |= {n for n, hit in (("empty first", (~full[:, 0] & some).any()), ("empty last", (~full[:, -1] & some).any()),
                                      ("only last", (full[:, -1] & (full.sum(axis=1) == 1)).any())) if hit}
    want = {"empty bag"} | ({"empty first", "empty last", "only last"} if hots.max() > 1 else set())
    assert seen == want, seen
    assert lone_special > 0
    for b in case["batches"]:      # the small batches see the patterns too (items 0 .. 2)
        assert (idx[:b] == -1).any()


def test_pooled_reference_rejects_a_fold_that_starts_from_zero(fr):
    """The reference itself tells a bit copy from `+0.0 + x`: on the case data, adding the first slot to +0.0 changes -0.0 rows, the
    signalling NaN's payload ... -- the words a kernel that folds from zero would get wrong."""
    case = next(c for c in G.POOLED_CASES if c["model"] == "mixed" and c["kernel"].endswith("<2, 4, false>"))
    m = G.make_model(fr, case["model"], case["mode"])
    tables, hots, idx, dense = G.pooled_data(m, case)
    want = G.pooled_expected(fr, m, tables, hots, idx, dense)
    orig = P.fold_slots

    def from_zero(slot_records, slot_valid):
        acc = np.zeros_like(slot_records[0], dtype=np.uint32)
        for v, ok in zip(slot_records, slot_valid):
            with np.errstate(all="ignore"):
                s = (acc.view(np.float32) + v.view(np.float32)).astype(np.float32).view(np.uint32)
            acc = np.where(ok, s, acc)
        return acc
    P.fold_slots = from_zero
    try:
        bad = G.pooled_expected(fr, m, tables, hots, idx, dense)
    finally:
        P.fold_slots = orig
    diff = bad != want
    assert diff.any()
    w = want[diff]
    assert (w == 0x80000000).any() and (w == 0x7FA12345).any()      # -0.0 became +0.0, the signalling NaN was quieted


# ---- the rounding helpers, pinned by something independent -------------------------------------------------------------------------------

def test_exhaustive_table_holds_what_it_promises():
    u = G.exhaustive_bits()
    assert u.shape == (6144, 64) and len(np.unique(u)) == 393216
    expo, mant = (u >> 23) & 0xFF, u & 0x7FFFFF
    nan = (expo == 255) & (mant != 0)
    assert int(nan.sum()) == 2 * 128 * 6 - 2                      # every upper half of exponent 255, less the two infinities: 1534
    assert int(((expo == 255) & (mant == 0)).sum()) == 2 and int(((u & 0x7FFFFFFF) == 0).sum()) == 2
    assert int(((expo == 0) & (mant != 0)).sum()) == 2 * 128 * 6 - 2     # fp32 subnormals
    assert int((((u & 0xFFFF) == 0x8000) & (expo != 255)).sum()) == 65280    # finite bf16 ties
    want, n = G.lp_expected(u, 1)
    assert np.array_equal(n, nan) and (want[u == 0x80000000] == 0x8000).all() and (want[u == 0x7F800000] == 0x7F80).all()
    assert (want[u == 0x7F7FFFFF] == 0x7F80).all()                # RNE carries the largest finite values into the infinity
    for e in (-8, 0, 3, 7):
        w8, _ = G.lp_expected(u, 2, e)
        assert (w8[u == 0x80000000] == 0x80).all() and (w8[u == 0x7F800000] == 0x7E).all() and (w8[u == 0xFF800000] == 0xFE).all()
        assert (w8[u == 0x7F7F0000] == 0x7E).all()                # a finite value whose product with the scale overflows
        assert ((w8[~nan] & 0x7F) != 0x7F).all()
    got = G.canon(np.array([0x7FC1, 0x7F80, 0xFFFF], np.uint16), np.array([True, True, True]), 1)
    assert got.tolist() == [G.NAN16, 0x7F80, G.NAN16]             # an infinity at a NaN input is not a NaN: it stays and fails


def test_rounding_helpers_match_torch_on_the_exhaustive_table():
    """bf16_round and e4m3_encode (finite values only) against torch's conversions, clamping first: 0 mismatches at the four exponents."""
    torch = pytest.importorskip("torch")
    if not hasattr(torch, "float8_e4m3fn"):
        pytest.skip("this torch has no float8_e4m3fn")
    u = G.exhaustive_bits().ravel()
    fin = ((u >> 23) & 0xFF) != 255
    x = u[fin].view(np.float32)
    t = torch.from_numpy(x.copy())
    ref16 = t.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal((bf16_round(x).view(np.uint32) >> 16).astype(np.uint16), ref16)
    for e in (-8, 0, 3, 7):
        with np.errstate(over="ignore"):
            xs = x * np.float32(2.0 ** e)
        ref8 = torch.from_numpy(xs.copy()).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
        got8 = e4m3_encode(xs)
        assert np.array_equal(got8, ref8), (e, int((got8 != ref8).sum()))
        assert len(np.unique(got8)) == 254 and int((np.abs(xs) > 448).sum()) > 150000


# ---- completeness ----------------------------------------------------------------------------------------------------------------------

def _library_kernels(fr):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources as KR
    finally:
        sys.path.pop(0)
    if not (os.path.exists(KR.READELF) or shutil.which("llvm-readelf")):
        pytest.skip("llvm-readelf not available")
    names = {E.demangle(r["name"]) for r in KR.kernel_records(fr.LIB_PATH)}
    if not names:
        pytest.skip("no gfx950 code objects found in %s" % fr.LIB_PATH)
    return names


def _is_fc_chain(n):
    return n.startswith(("fr_fused_tile", "fr_pipeline_kernel", "fr_gather_out_kernel")) or (n.startswith("fc_") and "gemm" in n)


def test_every_gather_kernel_is_named_by_a_case(fr):
    lib = {n for n in _library_kernels(fr) if n.startswith("gather_")}
    named = G.named_kernels()
    assert sorted(lib - named) == [], "gather kernels no case names"
    assert sorted(named - lib) == [], "names the library does not contain"
    assert len(lib) == 25


def test_every_other_kernel_is_covered_elsewhere(fr):
    """A kernel that is neither a gather kernel nor an FC-chain kernel is listed in COVERED_ELSEWHERE with the test that runs it."""
    rest = {n for n in _library_kernels(fr) if not n.startswith("gather_") and not _is_fc_chain(n)}
    assert sorted(rest - set(G.COVERED_ELSEWHERE)) == [], "kernels nobody has decided where to test"
    assert sorted(set(G.COVERED_ELSEWHERE) - rest) == [], "entries the library does not contain"


def test_covered_elsewhere_names_tests_that_exist():
    for kernel, where in G.COVERED_ELSEWHERE.items():
        path, _, fn = where.partition("::")
        src = open(os.path.join(ROOT, path)).read()
        assert "\ndef %s(" % fn in src, (kernel, where)

"""The table-sharded FC path on exact integer data (tests/exact_sharded.py), without a GPU: the premise of every (row, precision), the plan
properties each row relies on, the shard planner's guarantee (no empty shard; every plan that was clean keeps its bits:
tests/golden/shard_plans.json), the table-less shard, every fp32 row on the CPU back-end bit for bit, and simulated bugs of the slice re-pack
that the rows' data must see."""
import json
import os

import numpy as np
import pytest

import exact_chain as E
import exact_sharded as S

CPU = S.CPU
F32_ROWS = [r for r in S.ROWS if "f32" in r["precs"]]
PLANS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shard_plans.json")


def _plan_models(fr):
    models = {"builtin_A": fr.Model.builtin(fr.MODEL_A), "builtin_B": fr.Model.builtin(fr.MODEL_B), "builtin_C": fr.Model.builtin(fr.MODEL_C)}
    for name in ("A352", "B880", "C", "P"):
        models["exact_" + name] = S.model_data(fr, name)[0]
    return models


@pytest.mark.parametrize("r,prec", S.CELLS, ids=S.CELL_IDS)
def test_premise_holds(fr, r, prec):
    """Every fp32 summation order is exact on the row's batch in this precision, and from 32 items on the chain's roundings have work to do
    (asserted inside expect); the expectation is finite."""
    want, ae, we = S.expect(fr, r, prec)
    assert want.shape == (r["B"],) and np.isfinite(want).all()
    assert (ae is None) == (prec != "fp8")


@pytest.mark.parametrize("r", S.ROWS, ids=[r["id"] for r in S.ROWS])
def test_rows_sit_on_their_edges(fr, r):
    """What each row's `plan` states is what Model.shard_plan gives."""
    m = S.model_data(fr, r["model"])[0]
    facts = S.plan_facts(m, r)
    for key, val in r["plan"].items():
        assert facts[key] == val, (r["id"], key, facts[key], val)
    assert facts["min_len"] > 0
    if r["id"] == "d":   # two launches of the 64-shard slice table
        assert r["G"] > 64 > r["G"] - 64 and r["G"] > S.MAX_RANKS
    if r["id"] == "i":
        assert all((n + 31) // 32 * 32 == 4096 for n in facts["items"])


def test_planner_gives_every_shard_a_segment_and_keeps_clean_plans(fr):
    """No G in [1, n_segments] has an empty shard, the slices tile the record in order, and every plan the fixture lists (the plans without an empty
    shard before the planner guaranteed it) is unchanged."""
    with open(PLANS) as f:
        fixture = json.load(f)
    models = _plan_models(fr)
    assert sorted(fixture) == sorted(models)
    for name, m in models.items():
        fx = fixture[name]
        assert (fx["n_segments"], fx["record_len"]) == (m.desc.n_segments, m.record_len), name
        ends = set(s.rec_offset for s in m.segments()) | {m.record_len}
        for G in range(1, m.desc.n_segments + 1):
            offs, lens, F = m.shard_plan(G)
            assert min(lens) > 0, (name, G, lens)
            assert offs[0] == 0 and offs[-1] + lens[-1] == m.record_len and all(offs[g] + lens[g] == offs[g + 1] for g in range(G - 1)), (name, G)
            assert set(offs) <= ends and F == max(lens), (name, G)
            if str(G) in fx["plans"]:
                assert fx["plans"][str(G)] == [offs, lens, F], (name, G)
    # the plans the issue names as having held an empty shard are not in the fixture
    assert not {"6", "8", "9"} & set(fixture["exact_A352"]["plans"]) and "70" not in fixture["exact_C"]["plans"] and "131" not in fixture["builtin_C"]["plans"]
    with pytest.raises(fr.FleetRecError):
        models["exact_A352"].shard_plan(models["exact_A352"].desc.n_segments + 1)


def test_context_of_a_formerly_empty_shard_holds_its_segment(fr):
    """Row h's rank 3 (no segment before the fix): its context reports the plan's one-word slice and gathers it."""
    r = S.row("h")
    m, data, idx, dense, rec = S.batch(fr, r)
    offs, lens, F = m.shard_plan(r["G"])
    g = lens.index(4)
    c = fr.Context(m, device=CPU, shard_rank=g, n_shards=r["G"])
    wk = fr.Worker(c, r["B"])
    try:
        info = c.shard_info()
        assert (info["slice_offset"], info["slice_len"], info["slice_padded"]) == (offs[g], 4, F)
        for t in S.held_tables(m, offs[g], lens[g]):
            c.upload_table(t, data["tables"][t])
        sl = wk.gather_records(idx, dense).reshape(r["B"], F)
        assert np.array_equal(sl[:, :4], rec[:, offs[g]:offs[g] + 4].view(np.uint32))
    finally:
        wk.close()
        c.close()


def test_dense_only_shard_loads_by_upload(fr):
    S.check_dense_only_shard_loads_by_upload(fr, CPU)


@pytest.mark.parametrize("r", F32_ROWS, ids=[r["id"] for r in F32_ROWS])
def test_exact_sharded_row_on_the_cpu_backend(fr, r):
    S.check_row(fr, CPU, r, "f32")


def test_nan_table_value_on_the_cpu_backend(fr):
    S.check_nan_table_value(fr, CPU, "f32")


MUTANTS = [(r, name) for r in S.ROWS for name in r["mutants"]]


@pytest.mark.parametrize("r,name", MUTANTS, ids=["%s-%s" % (r["id"], name) for r, name in MUTANTS])
def test_simulated_repack_bugs_change_a_score(fr, r, name):
    """A bug of the slice re-pack, applied on the host to the gathered array or its assembly, changes at least one expected score of every row that
    targets its edge (else the row's data could not see it).  At most 64 items of one rank's range are restated."""
    m, data, idx, dense, rec = S.batch(fr, r)
    ws = data["ws"]
    offs, lens, F = m.shard_plan(r["G"])
    K = m.record_len
    if name == "fp8_pad":
        want, ae, we = S.expect(fr, r, "fp8")
        assert K % 64
        got = S.fp8_pad_mutant_scores(rec, ws, ae, we)
        assert not np.array_equal(got, want, equal_nan=True)
        return
    prec = "bf16" if name == "bf16_pair" else "f32"
    assert prec in r["precs"]
    want = S.expect(fr, r, prec)[0]
    gathered = S.host_gathered(rec, offs, lens, F)
    ranges = [(lo, hi - lo) for lo, hi in (S.item_range(g, r["G"], r["B"]) for g in range(r["G"]))]
    lo, n = next(((lo, n) for lo, n in ranges[1:] if n > 0), ranges[0]) if name == "item0" else ranges[0]
    n = min(n, 64)
    assert np.array_equal(S.assemble(gathered, offs, lens, K, lo, n), rec[lo:lo + n])   # the honest assembly gives the records
    bad = S.mutant_records(name, gathered, offs, lens, K, lo, n)
    assert bad is not None, "row %s has no place for the %s bug" % (r["id"], name)
    assert not np.array_equal(bad, rec[lo:lo + n])
    got = E.expected(prec, bad, ws)
    assert not np.array_equal(got, want[lo:lo + n]), "no score of row %s sees the %s bug" % (r["id"], name)

"""GPU parity of the sliced gather of the 64-item fp32 fused kernel (fr_fused_tile_m2_kernel<44>, fr_epi_tile_m2_kernel<44>): the kernel hands
record words 0 .. 23 to LDS, starts FC1's first chunk on groups 0 .. 11, and hands words 24 .. 55 and 56 .. 87 over behind two barriers in the
middle of that chunk.  Everything here is bit for bit: against the 32-item kernel (fr_fused_tile_kernel<2, 44, 4, false>, whose gather is ft_gather_tile,
untouched) on the same batches, and against the host's exact result on integer data (tests/exact_chain.py)."""
import numpy as np
import pytest

import exact_chain as E
from gpu_helpers import uniform_idx

pytestmark = pytest.mark.gpu

CUT_WORD = 24            # first record word of the second slice (4 floats per word); the third starts at word 56
M2, M2_EPI = "fr_fused_tile_m2_kernel<44>", "fr_epi_tile_m2_kernel<44>"
T32, T32_EPI = "fr_fused_tile_kernel<2, 44, 4, false>", "fr_epi_tile_kernel<2, 44, 2, true>"   # (a K = 352 context with an epilogue takes the <2, 44, 2, true> sibling)
B = 256
N_POOL = 8               # index / dense buffers: 0 .. 3 and 4 .. 7 are the two disjoint draws of the stale-Xq test


class Env:
    pass


@pytest.fixture(scope="module")
def env(fr, gpu):
    """A K = 352 user model (1024 / 512 / 256) whose 32 dense floats are record floats 80 .. 111 = words 20 .. 27: they straddle the slice
    boundary.  Small tables of 40 .. 30 000 rows, hashed contents, uniform weights, one worker."""
    rng = np.random.default_rng(97)
    dims = [8, 16, 4, 32, 20, 64, 4, 12, 8, 16, 24, 32, 48, 32]
    assert sum(dims) == 320 and sum(dims[:5]) == 80
    spec = {"name": "sliced_352", "dense_len": 32, "dense_at": 5, "fc": [1024, 512, 256],
            "tables": [{"dim": d_, "rows": int(rng.integers(40, 30000))} for d_ in dims]}
    e = Env()
    e.fr, e.m = fr, fr.Model.from_spec(spec)
    assert e.m.record_len == 352 and e.m.dense_len == 32
    dense_seg = [sg for sg in e.m.segments() if sg.kind == 2]
    assert len(dense_seg) == 1 and dense_seg[0].rec_offset < 4 * CUT_WORD < dense_seg[0].rec_offset + dense_seg[0].len
    e.ctx = fr.Context(e.m, device=gpu)
    e.ctx.fill_tables(fr.FILL_HASH, 5)
    e.ctx.fill_weights(fr.WEIGHTS_UNIFORM, 6)
    assert e.ctx.stream_group() == 64
    e.wk = fr.Worker(e.ctx, B)
    e.idx = [uniform_idx(rng, e.m.rows(), B) for _ in range(N_POOL)]
    e.dense = [rng.uniform(-1, 1, (B, 32)).astype(np.float32) for _ in range(N_POOL)]
    e.d_idx = [fr.DeviceBuffer.from_numpy(e.ctx, i_) for i_ in e.idx]
    e.d_dense = [fr.DeviceBuffer.from_numpy(e.ctx, d_) for d_ in e.dense]
    e.outs = [fr.DeviceBuffer(e.ctx, B * 4) for _ in range(128)]
    yield e
    e.wk.close()
    e.ctx.close()


def _run(e, group, plan, kernel):
    """Push plan = [(batch, pool entry)] at launch group `group` into NaN-filled buffers; -> the 256 floats of every buffer."""
    e.ctx.set_stream_group(group)
    try:
        for k, (b, j) in enumerate(plan):
            e.outs[k].upload(np.full(B, np.nan, np.float32))
        for k, (b, j) in enumerate(plan):
            e.wk.push_device(b, e.d_idx[j], e.d_dense[j], e.outs[k])
        assert e.wk.last_kernel() == kernel, e.wk.last_kernel()
        e.wk.sync()
        return [e.outs[k].download(np.float32, B) for k in range(len(plan))]
    finally:
        e.ctx.set_stream_group(64)


def _same_bits(got, want, plan, what):
    for k, (b, j) in enumerate(plan):
        assert np.array_equal(got[k][:b], want[k][:b]), (what, k, b, j)
        assert np.isfinite(got[k][:b]).all(), (what, k, b, j)
        assert np.isnan(got[k][b:]).all() and np.isnan(want[k][b:]).all(), (what, k, b, j)


def test_ragged_launch_bit_for_bit(env):
    """One full group of 64 batches sized from {256, 200, 77, 65, 64, 63, 1} (batches that end inside a tile, at a tile's edge, one item past
    it; whole tiles past the batch) through the 64-item kernel, and the same batches through the 32-item kernel at group 16."""
    sizes = [256, 200, 77, 256, 65, 256, 64, 200, 63, 256, 1, 256, 200, 256, 256, 200]
    plan = [(sizes[k % len(sizes)], k % 4) for k in range(64)]
    assert {b for b, _ in plan} == {256, 200, 77, 65, 64, 63, 1}
    assert sum((b + 63) // 64 for b, _ in plan) > 128
    got = _run(env, 64, plan, M2)
    want = _run(env, 16, plan, T32)
    _same_bits(got, want, plan, "ragged")


@pytest.mark.parametrize("epi", [False, True], ids=["plain", "epilogue"])
def test_late_rows_never_read_before_their_slice(env, epi):
    """Two full groups back to back on one worker, drawn from disjoint index and feature buffers: when a tile of the second launch starts, the
    late rows of Xq hold the record of the first launch's tile on that CU.  A group that reads them before the slice's barrier differs from the
    32-item kernel's scores of the same batches.  Once more with an epilogue on the context: the fr_epi_tile_m2_kernel<44> form."""
    plan = [(B, k % 4) for k in range(64)] + [(B, 4 + k % 4) for k in range(64)]
    rng = np.random.default_rng(11)
    try:
        if epi:
            for l, n in enumerate([1024, 512, 256]):
                env.ctx.set_epilogue(l, rng.uniform(-0.5, 0.5, n).astype(np.float32), "relu")
            env.ctx.set_epilogue(3, np.array([0.25], np.float32), "none")
        got = _run(env, 64, plan, M2_EPI if epi else M2)
        want = _run(env, 16, plan, T32_EPI if epi else T32)
        _same_bits(got, want, plan, "two groups")
        assert not np.array_equal(got[0], got[64])     # the two draws do give different scores
    finally:
        if epi:
            for l in range(4):
                env.ctx.set_epilogue(l, None, "none")


@pytest.mark.parametrize("table, item", [(0, 64), (0, 127), (13, 64), (13, 127)], ids=["first-slice-item0", "first-slice-item63", "last-slice-item0", "last-slice-item63"])
def test_range_flag_from_every_slice(env, table, item):
    """An out-of-range index in a table of the first slice (table 0: words 0, 1) and of the last slice (table 13: words 80 .. 87), at item 0 and
    at item 63 of a batch's second tile: the launch reports FR_ERR_INDEX_RANGE, and a clean launch afterwards is clean."""
    fr = env.fr
    bad = env.idx[0].copy()
    bad[item, table] = env.m.rows()[table]
    d_bad = fr.DeviceBuffer.from_numpy(env.ctx, bad)
    try:
        with pytest.raises(fr.FleetRecError) as err:
            for k in range(64):
                env.wk.push_device(B, d_bad if k == 37 else env.d_idx[k % 4], env.d_dense[k % 4], env.outs[k])
            assert env.wk.last_kernel() == M2
            env.wk.sync()
        assert err.value.status == fr.FR_ERR_INDEX_RANGE
        plan = [(B, k % 4) for k in range(64)]
        got = _run(env, 64, plan, M2)
        assert all(np.array_equal(got[k], got[k % 4]) and np.isfinite(got[k]).all() for k in range(64))
    finally:
        d_bad.free()


def test_exact_integer_data_every_word_distinct(fr, gpu):
    """Integer operands (tests/exact_chain.py) on tables in which the 88 record words of an item are 88 different 4-tuples: word w of row r
    holds the base-7 digits of 27 w + r % 27, shifted into [-3, 3].  A word stored to another word's Xq row, a slice handed over twice or a
    group of 8 k run twice changes an FC1 sum; the host's result is exact, so there is no tolerance.  64 batches of 256, each another
    rotation of the item pool, through fr_fused_tile_m2_kernel<44>."""
    sp = E.model_spec("A352")
    data = E.make_data(sp, E.model_seed("A352") + 1)
    m = fr.Model.from_spec(sp)
    for sg in m.segments():
        assert sg.kind != 2
        t = data["tables"][sg.src]
        r = np.arange(t.shape[0])[:, None]
        p = sg.rec_offset + np.arange(sg.len)[None, :]
        t[:, sg.src_col:sg.src_col + sg.len] = ((27 * (p // 4) + r % 27) // 7 ** (p % 4)) % 7 - 3
    idx = data["idx"][:B]
    rec = E.records(m, data, idx)
    words = rec.reshape(B, 88, 4)
    assert all(len({tuple(w_) for w_ in words[i]}) == 88 for i in range(B))
    E.premise("f32", rec, data["ws"])
    want = E.expected("f32", rec, data["ws"])
    ctx = fr.Context(m, device=gpu)
    wk = fr.Worker(ctx, B)
    try:
        E.load(ctx, data)
        assert ctx.stream_group() == 64
        d_idx = [fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(np.roll(idx, k, axis=0))) for k in range(64)]
        outs = [fr.DeviceBuffer(ctx, B * 4) for _ in range(64)]
        for k in range(64):
            wk.push_device(B, d_idx[k], None, outs[k])
        assert wk.last_kernel() == M2, wk.last_kernel()
        wk.sync()
        for k in range(64):
            assert np.array_equal(outs[k].download(np.float32, B), np.roll(want, k)), k
    finally:
        wk.close()
        ctx.close()

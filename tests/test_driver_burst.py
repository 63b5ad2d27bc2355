"""Short runs of the native driver loop (fr_driver_run_resident): a run is spread over no more workers than it has launch groups
(fr_ctx_stream_group), a run of one launch group goes inline on the calling thread to worker (0, 0), and the wrapper keeps the
marshalled pointer arrays of its last pool.  The expected scores come through Worker.push_device + sync, the same fused kernels the
driver launches (GPU), or Worker.infer (CPU back-end): every comparison is bit for bit."""
import numpy as np
import pytest

SEED_TABLES, SEED_WEIGHTS = 0xF1EE7, 99
CPU = -1
B = 256
THREADS, DEPTH = 2, 2


def uniform_idx(rng, rows, n):
    return (rng.random((n, len(rows))) * rows[None, :]).astype(np.int32)


def rings_of(drv, threads=THREADS, depth=DEPTH):
    return {(t, s): drv.score_ring(t, s, B) for t in range(threads) for s in range(depth)}


def nonzero_rows(ring):
    return np.flatnonzero(ring.any(axis=1))


# ------------------------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def burst(fr, gpu):
    """Model-A with 50 000-row tables, fp32, launch group 64, a pool of 8 distinct index buffers and their expected scores (batch 256 and
    the ragged batch 200), computed once."""
    m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=50000)
    ctx = fr.Context(m, device=gpu)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    ctx.set_stream_group(64)
    assert ctx.stream_group() == 64
    rng = np.random.default_rng(20)
    host = [uniform_idx(rng, m.rows(), B) for _ in range(8)]
    pool = [fr.DeviceBuffer.from_numpy(ctx, a) for a in host]
    wk = fr.Worker(ctx, B)
    out = [fr.DeviceBuffer(ctx, B * 4) for _ in pool]
    expect = {}
    for n in (B, 200):
        for p_, o_ in zip(pool, out):
            wk.push_device(n, p_, None, o_)
        wk.sync()
        expect[n] = [o_.download(np.float32, B)[:n].copy() for o_ in out]
    wk.close()
    for e in expect[B]:
        assert e.any()
    assert len({e.tobytes() for e in expect[B]}) == 8   # distinct, so a row names its pool entry
    yield fr, m, ctx, host, pool, expect
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("total", [1, 5, 20, 63, 64])
def test_burst_lands_in_the_first_workers_ring_in_id_order(burst, total):
    fr, m, ctx, host, pool, expect = burst
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    assert drv.run_resident(B, total, pool) > 0
    rings = rings_of(drv)
    drv.close()
    first = rings.pop((0, 0))
    assert list(nonzero_rows(first)) == list(range(total))
    for i in range(total):
        assert np.array_equal(first[i], expect[B][i % 8]), "row %d" % i
    for key, ring in rings.items():
        assert not ring.any(), "ring %r holds scores of a run of %d batches" % (key, total)


@pytest.mark.gpu
@pytest.mark.parametrize("total", [65, 129, 257, 403])
def test_longer_runs_use_no_more_workers_than_launch_groups(burst, total):
    fr, m, ctx, host, pool, expect = burst
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    assert drv.run_resident(B, total, pool) > 0
    rings = rings_of(drv)
    drv.close()
    known = {e.tobytes() for e in expect[B]}
    count, holders = 0, 0
    for key, ring in rings.items():
        nz = nonzero_rows(ring)
        count += len(nz)
        holders += 1 if len(nz) else 0
        for k in nz:
            assert ring[k].tobytes() in known, "ring %r row %d is no pool entry's scores" % (key, k)
    assert count == total
    assert holders <= -(-total // 64)


@pytest.mark.gpu
def test_ragged_batch_in_a_burst(burst):
    """batch 200 = 7 tiles of 32 items per batch, the last one partial."""
    fr, m, ctx, host, pool, expect = burst
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    assert drv.run_resident(200, 20, pool) > 0
    rings = rings_of(drv)
    drv.close()
    first = rings.pop((0, 0))
    assert list(nonzero_rows(first)) == list(range(20))
    for i in range(20):
        assert np.array_equal(first[i][:200], expect[200][i % 8]), "row %d" % i
        assert not first[i][200:].any()
    assert not any(r.any() for r in rings.values())


@pytest.mark.gpu
def test_out_of_range_index_in_a_burst_is_reported_and_the_driver_stays_usable(burst):
    fr, m, ctx, host, pool, expect = burst
    bad = host[3].copy()
    bad[17, 5] = m.rows()[5]   # one past the table's last row: the library reads row 0 instead and raises the worker's error word
    d_bad = fr.DeviceBuffer.from_numpy(ctx, bad)
    bad_pool = list(pool)
    bad_pool[3] = d_bad
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    with pytest.raises(fr.FleetRecError) as e:
        drv.run_resident(B, 20, bad_pool)
    assert e.value.status == fr.FR_ERR_INDEX_RANGE
    assert "driver thread 0" in str(e.value)
    assert drv.run_resident(B, 20, pool) > 0
    first = drv.score_ring(0, 0, B)
    drv.close()
    d_bad.free()
    for i in range(20):
        assert np.array_equal(first[i], expect[B][i % 8])


@pytest.mark.gpu
def test_launch_group_of_12_spreads_20_batches_over_two_workers(burst):
    fr, m, ctx, host, pool, expect = burst
    ctx.set_stream_group(12)
    try:
        drv = fr.Driver(ctx, THREADS, DEPTH, B)
        assert drv.run_resident(B, 20, pool) > 0
        rings = rings_of(drv)
        drv.close()
    finally:
        ctx.set_stream_group(64)
    # two workers = one thread, which draws the ids in order and alternates its two workers
    for s in range(2):
        ring = rings[(0, s)]
        assert list(nonzero_rows(ring)) == list(range(10))
        for j in range(10):
            assert np.array_equal(ring[j], expect[B][(2 * j + s) % 8]), "worker (0, %d) row %d" % (s, j)
    assert not rings[(1, 0)].any() and not rings[(1, 1)].any()


# ------------------------------------------------------------------------------------------------------------------
# CPU back-end (a group of 1: only a run of one batch goes inline on a driver with several workers)
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_burst(fr):
    m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=2000)
    ctx = fr.Context(m, device=CPU)
    ctx.fill_tables(fr.FILL_HASH, SEED_TABLES)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, SEED_WEIGHTS)
    assert ctx.stream_group() == 1
    rng = np.random.default_rng(21)
    host = [uniform_idx(rng, m.rows(), B) for _ in range(6)]
    wk = fr.Worker(ctx, B)
    want = [wk.infer(a).copy() for a in host]
    wk.close()
    assert len({w_.tobytes() for w_ in want}) == len(want) and all(w_.any() for w_ in want)
    yield fr, ctx, host, want
    ctx.close()


@pytest.mark.parametrize("total", [0, 1, 3, 4, 24])
def test_cpu_runs_of_every_length_leave_each_batch_once(cpu_burst, total):
    fr, ctx, host, want = cpu_burst
    n = 4
    pool = [fr.DeviceBuffer.from_numpy(ctx, a) for a in host[:n]]
    drv = fr.Driver(ctx, THREADS, DEPTH, B)
    assert drv.run_resident(B, total, pool) >= 0
    rings = rings_of(drv)
    drv.close()
    by_bytes = {w_.tobytes(): p for p, w_ in enumerate(want[:n])}
    seen = [0] * n
    for key, ring in rings.items():
        for k in nonzero_rows(ring):
            assert ring[k].tobytes() in by_bytes, "ring %r row %d is no pool entry's scores" % (key, k)
            seen[by_bytes[ring[k].tobytes()]] += 1
    assert sum(seen) == total
    assert seen == [len(range(p, total, n)) for p in range(n)]   # batch id -> pool entry id % n: every id ran exactly once
    if total == 1:   # one launch group: inline, worker (0, 0), slot 0
        assert np.array_equal(rings[(0, 0)][0], want[0])


def test_wrapper_keeps_its_pool_arrays_until_the_pool_changes(cpu_burst):
    fr, ctx, host, want = cpu_burst
    n = 4
    pool = [fr.DeviceBuffer.from_numpy(ctx, a) for a in host[:n]]
    drv = fr.Driver(ctx, 1, 1, B)   # one worker: ring row i is pool entry i % n

    def run():
        drv.run_resident(B, n, pool)
        return drv.score_ring(0, 0, B)[:n]

    r1 = run()
    arr = drv._pool_array("idx", pool)
    r2 = run()
    assert drv._pool_array("idx", pool) is arr   # the same list of the same buffers: marshalled once
    assert np.array_equal(r1, r2)
    for i in range(n):
        assert np.array_equal(r1[i], want[i])
    # an entry replaced in place by another buffer
    other = fr.DeviceBuffer.from_numpy(ctx, host[4])
    arr = drv._pool_array("idx", pool)
    pool[1] = other
    r3 = run()
    assert drv._pool_array("idx", pool) is not arr
    assert np.array_equal(r3[1], want[4])
    assert all(np.array_equal(r3[i], want[i]) for i in (0, 2, 3))
    # a buffer freed, a new one in its place (its address may well be the freed one's)
    pool[2].free()
    pool[2] = fr.DeviceBuffer.from_numpy(ctx, host[5])
    r4 = run()
    assert np.array_equal(r4[2], want[5])
    assert np.array_equal(r4[1], want[4]) and np.array_equal(r4[0], want[0]) and np.array_equal(r4[3], want[3])
    # the SAME object re-pointed: freed, then given a new allocation
    pool[0].free()
    fresh = fr.DeviceBuffer.from_numpy(ctx, host[1])
    pool[0].ptr, fresh.ptr = fresh.ptr, None
    r5 = run()
    assert np.array_equal(r5[0], want[1])
    drv.close()

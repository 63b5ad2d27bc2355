"""One create-use-destroy cycle over every owner of memory in the library (csrc/fr_mem.h), shared by tests/test_cpu_lifetime.py (device = -1, in
process) and tests/test_gpu_lifetime.py (a child process on the experiments build, which exports the tally of live bytes).  Everything is
released with close() / free(), never by the collector: after cycle() returns nothing of the library is alive."""
import numpy as np

B = 64   # max_batch of every worker


def rows_of(rng, m, n, slots=1):
    """n index rows of `slots` slots per index column, every id inside the column's table(s)"""
    lim = np.repeat(np.asarray(m.index_ranges(), dtype=np.int64), slots)
    return (rng.random((n, lim.size)) * lim[None, :]).astype(np.int32)


def dense_of(rng, m, n):
    return rng.uniform(-1, 1, (n, m.dense_len)).astype(np.float32) if m.dense_len else None


def make_ctx(fr, m, device, **kw):
    c = fr.Context(m, device=device, **kw)
    c.fill_tables(fr.FILL_HASH, 11)
    c.fill_weights(fr.WEIGHTS_UNIFORM, 5)
    return c


def sharded_steps(fr, m, device, rng):
    """G = 2 shard contexts on the one device (CPU: the host exchange; GPU: the staged exchange): a one-hot step in each exchange mode, then, created
    with their pooling, a pooled step in the padded and in the offsets form"""
    G, C = 2, m.idx_cols
    idx, dense = rows_of(rng, m, B), dense_of(rng, m, B)
    for hots in (None, [2] * C):
        ctxs = [make_ctx(fr, m, device, shard_rank=r, n_shards=G, hots=hots) for r in range(G)]
        wks = [fr.Worker(c, B) for c in ctxs]
        comms = fr.Comm.init_all(ctxs)
        got = []
        for step in (0, 1):
            if hots is None:
                for cm in comms:
                    cm.set_exchange(("allgather", "alltoall")[step])
                for w in wks:
                    w.idx[:B] = idx
                    if dense is not None:
                        w.dense[:B] = dense
                for r in range(G):
                    wks[r].submit_sharded(comms[r], B)
            else:
                pidx = rows_of(np.random.default_rng(23), m, B, 2)
                off, ind, _ = fr.bags_to_csr(pidx, hots)
                for r in range(G):
                    if step == 0:
                        wks[r].load_pooled(pidx, dense)
                        wks[r].submit_sharded_pooled(comms[r], B)
                    else:
                        wks[r].load_pooled_csr(off, ind, dense)
                        wks[r].submit_sharded_pooled_csr(comms[r], B)
            for w in wks:
                w.sync()
            got.append([w.score[:B].copy() for w in wks])
        assert all(np.array_equal(s, got[0][0]) for st in got for s in st), "the ranks or the two steps disagree"
        for x in wks + comms + ctxs:
            x.close()


def cycle(fr, m, device, idx, dense):
    """-> the fp32 scores of the fixed batch (idx, dense), taken first on a fresh context"""
    gpu = device >= 0
    rng = np.random.default_rng(17)
    C = m.idx_cols
    ctx = make_ctx(fr, m, device)
    wk = fr.Worker(ctx, B)
    fixed = wk.infer(idx, dense)
    for n_seg in (3, 9):   # host-form top-K: its pinned staging grows
        top, _ = wk.infer_topk(idx, 4, np.linspace(0, B, n_seg + 1).astype(np.int32), dense)
        assert top.shape == (n_seg, 4) and top.min() >= 0
    if gpu:
        out = [np.empty(B, np.float32) for _ in range(2)]   # the host ring, its events and its copy stream
        for o in out:
            wk.push_host(idx, dense, o)
        wk.sync()
        assert np.isfinite(out[0]).all() and np.array_equal(out[0], out[1])
        bufs = [fr.DeviceBuffer.from_numpy(ctx, idx)] + ([fr.DeviceBuffer.from_numpy(ctx, dense)] if dense is not None else [None])
        ctx.set_fc_precision(fr.FC_BF16)    # the bf16 weight copies ...
        d_sc = [ctx.buffer(B * 4) for _ in range(12)]
        for b in d_sc:                      # ... and a launch group of 12 batches (the persistent kernel's batch-list ring, where it takes the group)
            wk.push_device(B, bufs[0], bufs[1], b)
        wk.sync()
        sc = [b.download(np.float32, B) for b in d_sc]
        assert np.isfinite(sc[0]).all() and all(np.array_equal(s, sc[0]) for s in sc)
        ctx.set_fc_precision(fr.FC_FP8)     # the e4m3 copies and the reduction scratch
        ctx.set_fc_precision(fr.FC_FP32)
        n = 16385                           # more than one workgroup streams: the ranking's scratch
        d_s, d_top = fr.DeviceBuffer.from_numpy(ctx, rng.standard_normal(n).astype(np.float32)), ctx.buffer(8 * 4)
        wk.topk_device(n, d_s, 8, d_top)
        wk.sync()
        assert np.array_equal(np.sort(d_top.download(np.int32, 8)), np.sort(np.argsort(-d_s.download(np.float32, n), kind="stable")[:8]))
        for b in bufs + d_sc + [d_s, d_top]:
            if b is not None:
                b.free()
        mb = m.clone(index_mode=fr.INDEX_PER_BANK)   # a per-bank bf16 context with one push (the operand-type bank image where the launch reads one)
        cb = make_ctx(fr, mb, device)
        cb.set_fc_precision(fr.FC_BF16)
        wb = fr.Worker(cb, B)
        o = np.empty(B, np.float32)
        wb.push_host(rows_of(rng, mb, B), dense, o)
        wb.sync()
        assert np.isfinite(o).all()
        wb.close()
        cb.close()
    for n in (8, 64):   # the host form of the row update: its device staging grows
        t = m.desc.tables[0]
        ctx.update_rows(0, np.arange(n) % t.rows, np.full((n, t.dim), 0.5, np.float32))
    for hots in ([2] * C, [3] * C):   # the pooled descriptors, replaced once under a live worker (wk), a pooled worker for each
        ctx.set_pooling(hots)
        wp = fr.Worker(ctx, B)
        assert np.isfinite(wp.infer_pooled(rows_of(rng, m, B, hots[0]), dense)).all()
        wp.close()
    ctx.set_pooling(None)
    shared = np.zeros(C, np.int32)
    for first, dense_shared in ((0, m.dense_len > 0), (1, False)):   # the request split, replaced once, a worker created in between
        shared[:] = 0
        shared[first::2] = 1
        ctx.set_request_columns(shared, dense_shared)
        wr = fr.Worker(ctx, B)
        rs, rc, _ = ctx.request_words(fr.REQ_ONE_HOT)
        full = rows_of(rng, m, B)
        got = wr.infer_requests(full[:2, shared == 1], full[:, shared == 0], [0, 20, B], req_dense=dense[:2] if dense_shared else None,
                                dense=None if dense_shared else dense)
        assert (rs, rc) == (int(shared.sum()), C - int(shared.sum())) and np.isfinite(got).all()
        wr.close()
    ctx.set_request_columns(None)
    sharded_steps(fr, m, device, rng)
    busy = fr.Worker(ctx, B)   # destroyed with a batch in flight
    busy.idx[:B] = idx
    if dense is not None:
        busy.dense[:B] = dense
    busy.submit(B)
    busy.close()
    ctx.close()   # the worker outlives its context ...
    again = wk.infer(idx, dense)
    wk.close()    # ... and releases it
    assert np.isfinite(again).all()
    return fixed

"""Filtered bf16 retrieval (fr_ctx_set_retrieve_filter, fr_*_retrieve_filter_rows, fr_worker_retrieve_image_filtered_device / _filtered): the checks, stated
once in numpy and parameterised by device; the tests are tests/test_cpu_retrieve_filter.py (device = -1) and tests/test_gpu_retrieve_filter.py.  The
reference is tests/retrieve_lp.py's -- both operands rounded to bf16, tests/retrieve.py's float64 scores and ranking -- over the SURVIVING rows only.  All
data is integer-valued and bf16-exact: every comparison is bit for bit on rows and score bits."""
import os

import numpy as np

import rank_topk as R
import retrieve as T
import retrieve_lp as LP

CPU, C = T.CPU, T.C
ROWS = 3 * C + 5   # 96 whole tiles and a partial one; four chunks, the last of 5 rows
FILTER_LIB = os.path.join(R.ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_retrieve_filter.so")
# (dim, n_q, k, row0): the window ends with the table; it starts on a tile, inside one, on a tile's last row
MASK = [(dim, (1, 33)[(i + j) % 2], k, (0, 7, 31)[(i + j) % 3]) for i, dim in enumerate((4, 24, 128)) for j, k in enumerate((1, 3, 64, 256))]
# (k, live rows per chunk): chunk 1 is dead throughout and chunk 0 holds fewer than k; the last live row of chunk 3 scores NaN
MERGE = [(64, (10, 0, 20, 5)), (256, (10, 0, 300, 5)), (3, (2, 0, 0, 1)), (64, (0, 0, 0, 1)), (64, (0, 0, 0, 0))]


def context(fr, device, dim, rows=ROWS):
    m = fr.Model.from_spec({"name": "retrieve_filter", "tables": [{"dim": dim, "rows": rows}, {"dim": 4 if dim % 8 else 8, "rows": 16}], "fc": [32, 32, 32]})
    return m, fr.Context(m, device=device)


def reference(Q, Tab, row0, k, dead, excl):
    """the k best of every query over the window's rows that are neither in `dead` nor in the query's row of `excl` (or None)"""
    with np.errstate(invalid="ignore"):
        s64 = T.scores64(LP.bf16(Q), LP.bf16(Tab[row0:]))
    rows, sc = np.full((len(Q), k), -1, np.int32), np.full((len(Q), k), R.NEG_INF, np.uint32)
    for q in range(len(Q)):
        gone = np.concatenate([np.asarray(dead, np.int64), np.asarray(excl[q], np.int64) if excl is not None else np.zeros(0, np.int64)]) - row0
        keep = np.ones(s64.shape[1], bool)
        keep[gone[(gone >= 0) & (gone < len(keep))]] = False
        idx = np.flatnonzero(keep)
        r, s = T.reference(s64[q:q + 1, idx], 0, k)
        n = min(k, len(idx))
        rows[q, :n], sc[q] = row0 + idx[r[0, :n]], s[0]
    return rows, sc


def retrieve(fr, ctx, wk, Q, k, row0, excl=None, host=False, what="", rows=ROWS):
    """one filtered retrieval over table 0 from row0 to the table's end + sync -> (rows, score bits); the device form's outputs sit between canaries"""
    Q = np.ascontiguousarray(Q, np.float32)
    if host:
        rows, sc = wk.retrieve_image_filtered(0, Q, k, excl, row0)
        return rows, sc.view(np.uint32)
    d_q, out = fr.DeviceBuffer.from_numpy(ctx, Q), R.Outputs(fr, ctx, len(Q), k)
    d_x = None if excl is None else fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(excl, np.int32))
    try:
        wk.retrieve_image_filtered_device(0, row0, rows - row0, len(Q), d_q, 0 if excl is None else excl.shape[1], d_x, k, out.p_idx, out.p_sc)
        wk.sync()
        return out.read(what)
    finally:
        out.free()
        d_q.free()
        if d_x is not None:
            d_x.free()


def run_case(fr, device, Tab, Q, k, row0, dead, excl, host, what, by_worker=False):
    """upload, image, filter, the dead rows (with ids outside the table and a repeat, which do nothing), retrieve; against the reference"""
    rows = Tab.shape[0]
    m, ctx = context(fr, device, Tab.shape[1], rows)
    try:
        ctx.upload_table(0, Tab)
        ctx.set_retrieve_image(0)
        ctx.set_retrieve_filter(0)
        wk = fr.Worker(ctx, 16)
        ids = np.concatenate([np.asarray(dead, np.int32), np.array([-1, rows, rows + 31], np.int32), np.asarray(dead[:1], np.int32)])
        if by_worker:
            d_ids = fr.DeviceBuffer.from_numpy(ctx, ids)
            wk.retrieve_filter_rows(0, len(ids), d_ids, False)
        else:
            ctx.retrieve_filter_rows(0, ids, False)
        got = retrieve(fr, ctx, wk, Q, k, row0, excl, host, what, rows)
        if by_worker:
            d_ids.free()
        wk.close()
    finally:
        ctx.close()
    want = reference(Q, Tab, row0, k, dead, excl)
    R.assert_same(got, want, what)
    return got, want


def integers(seed, dim, n_q):
    """retrieve_lp.exact_case's data: integers in [-4, 4] and a few +-257 / +-259, which a conversion that is not round-to-nearest-even misses"""
    rng = np.random.default_rng(seed)
    Tab, Q = rng.integers(-4, 5, (ROWS, dim)).astype(np.float32), rng.integers(-4, 5, (n_q, dim)).astype(np.float32)
    Tab[40, 0], Tab[ROWS // 2, dim - 1], Tab[ROWS - 2, 1] = 259, -257, 257
    Q[0, 0], Q[-1, dim - 1], Q[n_q // 2, 1] = 259, -259, 257
    return Tab, Q


def mask_case(fr, device, dim, n_q, k, row0):
    """dead: a tile's first and last row, a whole tile, the window's first and last row, two rows of the partial last tile, the row in front of the window"""
    Tab, Q = integers(8100 + dim + k, dim, n_q)
    dead = [64, 95, *range(128, 160), row0, ROWS - 1, 3 * C + 1, max(row0 - 1, 0), 2 * C, 2 * C - 1]
    return run_case(fr, device, Tab, Q, k, row0, dead, None, (dim + k + n_q) % 2 == 0, str((dim, n_q, k, row0)), by_worker=k == 3)[0]


def merge_case(fr, device, k, live):
    """the lists of the four chunks hold live[c] rows each: pads in front of real entries of later chunks, and a real NaN among them"""
    Tab, Q = integers(8200 + k, 4, 2)
    alive = [c * C + 3 + 3 * i for c in range(3) for i in range(live[c])] + list(range(ROWS - live[3], ROWS))
    Tab[ROWS - 1] = np.nan
    got, want = run_case(fr, device, Tab, Q, k, 0, sorted(set(range(ROWS)) - set(alive)), None, False, "merge %s" % (live,))
    n = sum(live)
    if 0 < n <= k:
        assert (want[0][:, n - 1] == ROWS - 1).all() and (want[1][:, n - 1] == T.QNAN).all()   # the NaN row: behind every real score, before every pad
    assert (want[0][:, n:] == -1).all() and (want[1][:, n:] == R.NEG_INF).all() and (want[0][:, :min(n, k)] >= 0).all()
    return got


def long_case(fr, device):
    """17 chunks at k = 256: 4352 composites per query, more than one merge workgroup streams -- the stretches' leaders are folded by a second launch.
    The best rows sit in the first and in the last chunk; a tile of every chunk is dead"""
    rows, rng = 17 * C - 3, np.random.default_rng(8250)
    Tab, Q = rng.integers(-4, 5, (rows, 4)).astype(np.float32), rng.integers(1, 5, (2, 4)).astype(np.float32)
    Tab[[5, rows - 2]] = 100
    dead = [c * C + 32 + i for c in range(17) for i in range(32) if c * C + 32 + i < rows]
    got, want = run_case(fr, device, Tab, Q, 256, 3, dead, np.array([[5], [-1]], np.int32), False, "17 chunks")
    assert want[0][:, 0].tolist() == [rows - 2, 5]
    return got


def exclude_case(fr, device, n_excl):
    """per query: its best row, its k-th, a dead row, -1, a row in front of the window, the best once more; two query tiles, every list its own"""
    k, row0, dead = 64, 7, [100, 101, 2 * C + 9]
    Tab, Q = integers(8300 + n_excl, 24, 33)
    plain = reference(Q, Tab, row0, k, dead, None)[0]
    excl = np.full((33, n_excl), -1, np.int32)
    for q in range(33):
        named = [plain[q, 0], plain[q, k - 1], 100, -1, 3, plain[q, 0]] + list(plain[q, 1:k:2])
        excl[q, :min(n_excl, len(named))] = named[:n_excl]
    assert len({tuple(x) for x in excl.tolist()}) > 1
    got, want = run_case(fr, device, Tab, Q, k, row0, dead, excl, n_excl == 1, "n_excl %d" % n_excl)
    assert (want[0][:, 0] != plain[:, 0]).all()
    return got


def adversarial_case(fr, device):
    """retrieve_lp.adversarial_case's ramps at k = 256 with every query's 64 best rows excluded: every round appends, reduces and looks at the lists"""
    Tab, Q = np.zeros((ROWS, 4), np.float32), np.zeros((3, 4), np.float32)
    Tab[:, 0], Tab[:, 1], Tab[:, 2] = np.arange(ROWS) // 64 - 24, 1, np.arange(ROWS) % 64
    Q[0, 0], Q[0, 2], Q[2, 1] = 64, 1, 1
    Q[1] = -Q[0]
    excl = np.stack([np.arange(ROWS - 64, ROWS), np.arange(7, 71), np.arange(7, 71)]).astype(np.int32)
    got, want = run_case(fr, device, Tab, Q, 256, 7, [], excl, False, "adversarial")
    assert list(want[0][0][:2]) == [ROWS - 65, ROWS - 66] and list(want[0][1][:2]) == [71, 72] and list(want[0][2][:2]) == [71, 72]
    return got


def check_equivalence_and_stream_order(fr, device):
    """hash-filled rows.  Every row live and no exclusions: the image call's rows and bits.  Then push a batch -> rows dead -> filtered retrieve -> live
    again -> retrieve, no sync in between: the first lacks exactly the dead rows, the second is the image call's, the batch keeps its scores; dropping the
    filter under the un-synchronised retrieval is refused.  Then the context form in front of a retrieval."""
    rng = np.random.default_rng(8500)
    n_q, k, row0 = 33, 64, 7
    m, ctx = context(fr, device, 32)
    try:
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
        ctx.set_retrieve_image(0)
        ctx.set_retrieve_filter(0)
        wk = fr.Worker(ctx, 64)
        Q = rng.uniform(-1, 1, (n_q, 32)).astype(np.float32)
        base = LP.retrieve(fr, ctx, wk, Q, k + 32, row0, ROWS - row0, what="image")   # 32 more than k: what is left when up to 32 rows die
        R.assert_same(retrieve(fr, ctx, wk, Q, k + 32, row0, what="all live"), base, "every row live, no exclusions: the image call")
        R.assert_same(retrieve(fr, ctx, wk, Q, k + 32, row0, host=True), base, "the host form")
        dead = np.unique(base[0][:2, :2]).astype(np.int32)   # the two best rows of queries 0 and 1

        def without(dead):
            rows, bits = np.empty((n_q, k), np.int32), np.empty((n_q, k), np.uint32)
            for q in range(n_q):
                keep = ~np.isin(base[0][q], dead)
                rows[q], bits[q] = base[0][q][keep][:k], base[1][q][keep][:k]
            return rows, bits

        idx = np.stack([rng.integers(0, 2000, 64), rng.integers(0, 16, 64)], axis=1).astype(np.int32)
        plain = wk.infer(idx).view(np.uint32).copy()
        d_idx, d_sc = fr.DeviceBuffer.from_numpy(ctx, idx), fr.DeviceBuffer.from_numpy(ctx, np.zeros(64, np.uint32))
        d_dead, d_q = fr.DeviceBuffer.from_numpy(ctx, dead), fr.DeviceBuffer.from_numpy(ctx, Q)
        out1, out2 = R.Outputs(fr, ctx, n_q, k), R.Outputs(fr, ctx, n_q, k)
        wk.push_device(64, d_idx, None, d_sc)
        wk.retrieve_filter_rows(0, len(dead), d_dead, False)
        wk.retrieve_image_filtered_device(0, row0, ROWS - row0, n_q, d_q, 0, None, k, out1.p_idx, out1.p_sc)
        wk.retrieve_filter_rows(0, len(dead), d_dead, True)
        wk.retrieve_image_filtered_device(0, row0, ROWS - row0, n_q, d_q, 0, None, k, out2.p_idx, out2.p_sc)
        if device != CPU:
            assert fr.lib().fr_ctx_set_retrieve_filter(ctx._h, 0, fr.RETRIEVE_FILTER_NONE) == fr.FR_ERR_STATE and b"in flight" in fr.lib().fr_last_error()
        wk.sync()
        R.assert_same(out1.read("dead"), without(dead), "rows dead in front of the retrieval")
        R.assert_same(out2.read("live again"), without([]), "rows live again in front of the retrieval")
        assert np.array_equal(d_sc.download(np.uint32, 64), plain)
        ctx.retrieve_filter_rows(0, base[0][:16, 0], False)
        R.assert_same(retrieve(fr, ctx, wk, Q, k, row0), without(base[0][:16, 0]), "the context form")
        ctx.set_retrieve_filter(0)   # every row live again, in place
        R.assert_same(retrieve(fr, ctx, wk, Q, k, row0), without([]), "a second ROWS call")
        ctx.set_retrieve_filter(0, fr.RETRIEVE_FILTER_NONE)
        for b in (d_idx, d_sc, d_dead, d_q):
            b.free()
        out1.free(), out2.free()
        wk.close()
    finally:
        ctx.close()


# name -> (what is set up first: image / filter, the arguments that differ from a good call, the status, a word of the error text)
REFUSALS = {
    "no filter": ("i", {}, "STATE", "no retrieval filter"), "no image": ("f", {}, "STATE", "no retrieval image"), "n_excl -1": ("if", dict(n_excl=-1), "INVALID", "n_excl"),
    "n_excl 65": ("if", dict(n_excl=65), "INVALID", "n_excl"), "NULL exclude": ("if", dict(x=None), "INVALID", "exclude is NULL"), "k 0": ("if", dict(k=0), "INVALID", "k = 0"),
    "window past the table": ("if", dict(row0=ROWS - 9), "INVALID", "window"), "table out of range": ("if", dict(table=2), "INVALID", "out of range"),
}


def check_refusal(fr, device, name):
    """status, the text in fr_last_error, and both outputs untouched behind a following sync"""
    have, bad, status, word = REFUSALS[name]
    m, ctx = context(fr, device, 8)
    try:
        L = fr.lib()
        wk = fr.Worker(ctx, 16)
        if "i" in have:
            ctx.set_retrieve_image(0)
        if "f" in have:
            ctx.set_retrieve_filter(0)
        d_q, out = fr.DeviceBuffer.from_numpy(ctx, np.ones((2, 8), np.float32)), R.Outputs(fr, ctx, 2, 4)
        d_x = fr.DeviceBuffer.from_numpy(ctx, np.full((2, 65), -1, np.int32))
        a = dict(table=0, row0=0, n_rows=10, n_q=2, n_excl=2, x=d_x.ptr, k=4)
        a.update(bad)
        for entry in (L.fr_worker_retrieve_image_filtered_device, L.fr_worker_retrieve_image_filtered):
            got = entry(wk._h, a["table"], a["row0"], a["n_rows"], a["n_q"], d_q.ptr, a["n_excl"], a["x"], a["k"], out.p_idx, out.p_sc)
            assert got == getattr(fr, "FR_ERR_" + status) and word in L.fr_last_error().decode(), (name, got, L.fr_last_error())
        wk.sync()
        rows, bits = out.read(name)
        assert (rows.view(np.uint32) == R.CANARY).all() and (bits == R.CANARY).all(), "a refused call wrote its outputs"
        for b in (d_q, d_x):
            b.free()
        out.free()
        wk.close()
    finally:
        ctx.close()


def check_filter_refusals(fr, device):
    """fr_ctx_set_retrieve_filter and both fr_*_retrieve_filter_rows: every refusal of their own"""
    m, ctx = context(fr, device, 8)
    try:
        L, E = fr.lib(), lambda s: getattr(fr, "FR_ERR_" + s)
        wk = fr.Worker(ctx, 16)
        d_ids = fr.DeviceBuffer.from_numpy(ctx, np.arange(4, dtype=np.int32))
        assert L.fr_ctx_set_retrieve_filter(ctx._h, 0, 2) == E("INVALID") and L.fr_ctx_set_retrieve_filter(ctx._h, 2, 1) == E("INVALID")
        assert L.fr_ctx_set_retrieve_filter(ctx._h, 0, fr.RETRIEVE_FILTER_NONE) == fr.FR_OK   # (nothing to free)
        for entry, h in ((L.fr_worker_retrieve_filter_rows, wk._h), (L.fr_ctx_retrieve_filter_rows, ctx._h)):
            assert entry(h, 0, 4, d_ids.ptr, 1) == E("STATE") and "no retrieval filter" in L.fr_last_error().decode()
        ctx.set_retrieve_filter(0)
        for entry, h in ((L.fr_worker_retrieve_filter_rows, wk._h), (L.fr_ctx_retrieve_filter_rows, ctx._h)):
            assert entry(h, 0, 4, None, 1) == E("INVALID") and entry(h, 0, 4, d_ids.ptr, 2) == E("INVALID") and entry(h, 0, -1, d_ids.ptr, 1) == E("INVALID")
            assert entry(h, 2, 4, d_ids.ptr, 1) == E("INVALID") and entry(h, 0, 0, None, 0) == fr.FR_OK
        wk.sync()
        d_ids.free()
        wk.close()
    finally:
        ctx.close()
    big = fr.Context(T.model(fr, 8, 256), device=device)
    try:
        assert fr.lib().fr_ctx_set_retrieve_filter(big._h, 1, 1) == fr.FR_ERR_STATE and "dim 256" in fr.lib().fr_last_error().decode()
    finally:
        big.close()


def check_companion(fr):
    """libfleetrec_retrieve_filter.so (companion.check_companion): the mask kernel, two scan and two merge instantiations (KP = 64 / 256).  No VGPR cap,
    as for the other scans."""
    import companion
    companion.check_companion(fr, FILTER_LIB, ["fr_retrieve_filter_mask_launch", "fr_retrieve_filter_merge_launch", "fr_retrieve_filter_scan_launch"],
                              {"retrieve_filter_mask_kernel": 1, "retrieve_filter_scan_kernel": 2, "retrieve_filter_merge_kernel": 2}, "retrieve_filter_",
                              (fr.LIB_PATH, R.RANK_LIB, T.RETRIEVE_LIB, LP.LP_LIB), max_vgprs=None)

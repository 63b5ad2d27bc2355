"""bf16 retrieval over a table image (fr_ctx_set_retrieve_image, fr_worker_retrieve_image_device / fr_worker_retrieve_image): the checks, stated once in
numpy and parameterised by device; the tests are tests/test_cpu_retrieve_lp.py (device = -1) and tests/test_gpu_retrieve_lp.py.  The reference is the
contract in numpy: both operands rounded to bf16 (nearest even), then tests/retrieve.py's float64 scores and ranking."""
import os

import numpy as np

import rank_topk as R
import retrieve as T

CPU, C, ROWS = T.CPU, T.C, T.ROWS   # ROWS = 3C + 16 is no multiple of 32: the table's last tile is partial
LP_LIB = os.path.join(R.ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_retrieve_lp.so")
# (dim, n_q, k, n_rows, row0): every n_rows x every dim, the other three rotated as retrieve.EXACT rotates them.  dim: a pad inside the only step, one
# step, a step and a half, the maximum; row0: tile-aligned, inside a tile, the last row of a tile (the largest window starts where the table lets it: 11)
EXACT = [(dim, (1, 31, 33)[(i + j) % 3], (1, 3, 64, 256)[(i + 2 * j) % 4], n_rows, min((0, 7, 63)[(i + j) % 3], ROWS - n_rows))
         for i, n_rows in enumerate((1, 31, 33, C - 1, C + 1, 3 * C + 5)) for j, dim in enumerate((4, 12, 16, 24, 128))]
ADVERSARIAL = [(4, 256), (128, 64)]


def bf16(x):
    """fp32 -> the nearest bf16 value (ties to even), as fp32; a NaN stays a NaN"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)
    return np.where(np.isnan(x), x, r)


def retrieve(fr, ctx, wk, Q, k, row0, n_rows, host=False, what=""):
    """one image retrieval over table 0 + sync -> (rows, score bits); the device form's outputs sit between canaries"""
    Q = np.ascontiguousarray(Q, np.float32)
    if host:
        rows, sc = wk.retrieve_image(0, Q, k, row0, n_rows)
        return rows, sc.view(np.uint32)
    d_q, out = fr.DeviceBuffer.from_numpy(ctx, Q), R.Outputs(fr, ctx, len(Q), k)
    try:
        wk.retrieve_image_device(0, row0, n_rows, len(Q), d_q, k, out.p_idx, out.p_sc)
        wk.sync()
        return out.read(what)
    finally:
        out.free()
        d_q.free()


def run_case(fr, device, Tab, Q, k, row0, n_rows, host, what):
    """upload, build the image, retrieve; against the reference over the rounded operands"""
    m, ctx = T.context(fr, device, Tab.shape[1])
    try:
        ctx.upload_table(0, Tab)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        got = retrieve(fr, ctx, wk, Q, k, row0, n_rows, host=host, what=what)
        wk.close()
    finally:
        ctx.close()
    with np.errstate(invalid="ignore"):
        want = T.reference(T.scores64(bf16(Q), bf16(Tab[row0:row0 + n_rows])), row0, k)
    R.assert_same(got, want, what)
    return got, want


def exact_case(fr, device, dim, n_q, k, n_rows, row0):
    """integers in [-4, 4] and a few +-257 / +-259 (bf16: 256 and 260 -- an fp32 scan and a truncating conversion both miss): every partial sum stays
    far below 2^24, so every fp32 sum is exact in any order; the host form takes every other case"""
    rng = np.random.default_rng(7100 + dim + n_rows)
    Tab, Q = rng.integers(-4, 5, (ROWS, dim)).astype(np.float32), rng.integers(-4, 5, (n_q, dim)).astype(np.float32)
    Tab[row0, 0], Tab[row0 + n_rows // 2, dim - 1], Tab[row0 + n_rows - 1, 1] = 259, -257, 257
    Q[0, 0], Q[-1, dim - 1], Q[n_q // 2, 1] = 259, -259, 257
    return run_case(fr, device, Tab, Q, k, row0, n_rows, (n_rows + n_q) % 2 == 0, str((dim, n_q, k, n_rows, row0)))[0]


def adversarial_case(fr, device, dim, k):
    """row r = 64 a + b holds (a, 1, b): query (64, 0, 1) ascends strictly with the row (every tile beats the threshold), its negative descends, (0, 1, 0)
    is all equal -- the orders of retrieve.adversarial_case with bf16-exact operands"""
    Tab, Q = np.zeros((ROWS, dim), np.float32), np.zeros((3, dim), np.float32)
    Tab[:, 0], Tab[:, 1], Tab[:, 2] = np.arange(ROWS) // 64 - 24, 1, np.arange(ROWS) % 64
    Q[0, 0], Q[0, 2], Q[2, 1] = 64, 1, 1
    Q[1] = -Q[0]
    got, want = run_case(fr, device, Tab, Q, k, 7, 3 * C + 5, False, "adversarial order, dim %d, k %d" % (dim, k))
    assert list(want[0][0][:2]) == [7 + 3 * C + 4, 7 + 3 * C + 3] and list(want[0][1][:2]) == [7, 8] and list(want[0][2][:2]) == [7, 8]
    return got


def check_special(fr, device):
    """retrieve.check_special's table through the image path: a NaN row, +inf, -inf, a +0, a -0 and a mixed-zero row; k = 64 > 40 rows"""
    rng = np.random.default_rng(6300)
    Tab = rng.integers(-4, 5, (ROWS, 4)).astype(np.float32)
    Tab[11], Tab[20], Tab[21], Tab[30], Tab[31], Tab[32] = np.nan, (np.inf, 1, 1, 1), (-np.inf, 1, 1, 1), 0.0, -0.0, (0.0, -0.0, 0.0, -0.0)
    Q = np.array([[1, 2, 1, 3], [-1, -2, -1, -3]], np.float32)
    got, want = run_case(fr, device, Tab, Q, 64, 7, 40, False, "special values")
    assert (want[1] == 0x80000000).any() and (want[1] == 0).any() and (want[1] == T.QNAN).any()
    assert want[0][0][0] == 20 and list(want[0][0][38:41]) == [21, 11, -1]     # +inf first; -inf, the NaN row, then the padding


def check_rounded(fr, device, dim):
    """hash-filled rows, uniform queries, in the shape of retrieve.check_rounded: against the float64 scores of the ROUNDED operands the fp32 sum of `dim`
    exact products is within dim 2^-24 sum |q t| in any order"""
    n_q, k, row0, n_rows = 33, 64, 7, 3 * C + 5
    m, ctx = T.context(fr, device, dim)
    try:
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_image(0)
        Tab = bf16(ctx.download_table(0, row0, n_rows, np.float32))
        Q = np.random.default_rng(7400 + dim).uniform(-1, 1, (n_q, dim)).astype(np.float32)
        wk = fr.Worker(ctx, 16)
        rows, bits = retrieve(fr, ctx, wk, Q, k, row0, n_rows, what="rounded")
        wk.close()
    finally:
        ctx.close()
    Q = bf16(Q)
    s64 = T.scores64(Q, Tab)
    bound = dim * 2.0 ** -24 * (np.abs(Q.astype(np.float64)) @ np.abs(Tab.astype(np.float64)).T)
    q = np.arange(n_q)[:, None]
    assert (rows >= row0).all() and (rows < row0 + n_rows).all() and all(len(set(r)) == k for r in rows.tolist())
    err = np.abs(bits.view(np.float32).astype(np.float64) - s64[q, rows - row0])
    print("dim %d: largest error / bound %.3f" % (dim, (err / bound[q, rows - row0]).max()))
    assert (err <= bound[q, rows - row0]).all()
    key = R.keys(bits).astype(np.int64)
    assert ((key[:, 1:] < key[:, :-1]) | ((key[:, 1:] == key[:, :-1]) & (rows[:, 1:] > rows[:, :-1]))).all()
    left = np.ones(s64.shape, bool)
    left[q, rows - row0] = False
    kth, kth_bound = s64[q, rows[:, -1:] - row0], bound[q, rows[:, -1:] - row0]
    assert not (left & (s64 - kth > bound + kth_bound)).any()   # fp32(left out) <= fp32(k-th), each within its own bound


def check_patch(fr, device):
    """push a batch, update rows (row 17 twice with two contents -- whichever the scatter keeps, both images read it back --, row 0, the table's last row in its partial tile; row 2500 is made to win), retrieve over
    the image -- no sync in between: the new rows rank first, the batch still gets its scores; a rebuild then gives the same rows and bits"""
    rng = np.random.default_rng(7500)
    m, ctx = T.context(fr, device, 32)
    try:
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 64)
        idx = np.stack([rng.integers(0, 2000, 64), rng.integers(0, 16, 64)], axis=1).astype(np.int32)
        plain = wk.infer(idx).view(np.uint32).copy()
        Q = rng.uniform(0.5, 1, (2, 32)).astype(np.float32)
        ids = np.array([17, 2500, 0, ROWS - 1, 17], np.int32)
        new = np.repeat(np.array([3, 100, 50, 60, -3], np.float32)[:, None], 32, axis=1)
        d_idx, d_sc = fr.DeviceBuffer.from_numpy(ctx, idx), fr.DeviceBuffer.from_numpy(ctx, np.zeros(64, np.uint32))
        d_id, d_row = fr.DeviceBuffer.from_numpy(ctx, ids), fr.DeviceBuffer.from_numpy(ctx, new)
        d_q, out = fr.DeviceBuffer.from_numpy(ctx, Q), R.Outputs(fr, ctx, 2, 64)
        wk.push_device(64, d_idx, None, d_sc)
        wk.update_rows(0, len(ids), d_id, d_row)
        wk.retrieve_image_device(0, 0, ROWS, 2, d_q, 64, out.p_idx, out.p_sc)
        wk.sync()
        rows, bits = out.read("patched image")
        assert rows[:, :3].tolist() == [[2500, ROWS - 1, 0]] * 2
        qsum = bf16(Q).astype(np.float64).sum(1)
        assert (np.abs(bits[:, 0].view(np.float32) - 100 * qsum) <= 32 * 2.0 ** -24 * 100 * qsum).all()
        assert np.array_equal(d_sc.download(np.uint32, 64), plain)
        ctx.set_retrieve_image(0)
        wk.retrieve_image_device(0, 0, ROWS, 2, d_q, 64, out.p_idx, out.p_sc)
        wk.sync()
        R.assert_same(out.read("rebuilt image"), (rows, bits), "a patched image and a rebuilt one")
        for b in (d_idx, d_sc, d_id, d_row, d_q):
            b.free()
        out.free()
        wk.close()
    finally:
        ctx.close()


def _set(fr, ctx, table, kind, status, word):
    assert fr.lib().fr_ctx_set_retrieve_image(ctx._h, table, kind) == getattr(fr, "FR_ERR_" + status) and word in fr.lib().fr_last_error().decode()


# name -> (what makes the context, what happens before the retrievals, the arguments that differ from a good call, their status, a word of the error text)
STEPS = {
    "": lambda fr, ctx: None,
    "set": lambda fr, ctx: ctx.set_retrieve_image(0),
    "upload": lambda fr, ctx: (ctx.set_retrieve_image(0), ctx.upload_table(0, np.ones((1, 8), np.float32), 5)),
    "fill": lambda fr, ctx: (ctx.set_retrieve_image(0), ctx.fill_tables(fr.FILL_HASH, 7)),
    "none": lambda fr, ctx: (ctx.set_retrieve_image(0), ctx.set_retrieve_image(0, fr.RETRIEVE_IMAGE_NONE)),
    "kind 2": lambda fr, ctx: _set(fr, ctx, 0, 2, "INVALID", "kind 2"),
    "table 2": lambda fr, ctx: _set(fr, ctx, 2, 1, "INVALID", "out of range"),
    "dim 256": lambda fr, ctx: _set(fr, ctx, 1, 1, "STATE", "dim 256"),
    "sharded": lambda fr, ctx: _set(fr, ctx, 0, 1, "STATE", "sharded"),
    "per bank": lambda fr, ctx: _set(fr, ctx, 0, 1, "STATE", "PER_BANK"),
}
REFUSALS = {
    "no image": ({}, "", {}, "STATE", "no retrieval image"), "stale after upload_table": ({}, "upload", {}, "STATE", "stale"),
    "stale after fill_tables": ({}, "fill", {}, "STATE", "stale"), "NONE then retrieve": ({}, "none", {}, "STATE", "no retrieval image"),
    "kind 2": ({}, "kind 2", {}, "STATE", "no retrieval image"), "table out of range": ({}, "table 2", dict(table=2), "INVALID", "out of range"),
    "k 0": ({}, "set", dict(k=0), "INVALID", "k = 0"), "k 257": ({}, "set", dict(k=257), "INVALID", "k = 257"),
    "n_q 0": ({}, "set", dict(n_q=0), "INVALID", "n_q"), "n_q 65537": ({}, "set", dict(n_q=65537), "INVALID", "n_q"),
    "n_rows 0": ({}, "set", dict(n_rows=0), "INVALID", "window"), "window past the table": ({}, "set", dict(row0=ROWS - 9), "INVALID", "window"),
    "dim 256": (dict(extra_dim=256), "dim 256", dict(table=1, n_rows=8), "STATE", "dim 256"), "sharded": (dict(n_shards=2), "sharded", {}, "STATE", "sharded"),
    "per bank": (dict(per_bank=True), "per bank", {}, "STATE", "PER_BANK"),
}


def check_refusal(fr, device, name):
    """status, the text in fr_last_error, and both outputs untouched behind a following sync"""
    make, step, bad, status, word = REFUSALS[name]
    m = T.model(fr, 8, make.get("extra_dim"))
    if make.get("per_bank"):
        m = m.clone(index_mode=fr.INDEX_PER_BANK)
    ctx = fr.Context(m, device=device, n_shards=make.get("n_shards", 1))
    try:
        L = fr.lib()
        wk = fr.Worker(ctx, 16)
        STEPS[step](fr, ctx)
        d_q, out = fr.DeviceBuffer.from_numpy(ctx, np.ones((2, 256), np.float32)), R.Outputs(fr, ctx, 2, 4)
        a = dict(table=0, row0=0, n_rows=10, n_q=2, k=4)
        a.update(bad)
        for entry in (L.fr_worker_retrieve_image_device, L.fr_worker_retrieve_image):
            got = entry(wk._h, a["table"], a["row0"], a["n_rows"], a["n_q"], d_q.ptr, a["k"], out.p_idx, out.p_sc)
            assert got == getattr(fr, "FR_ERR_" + status), (name, got)
            assert word in L.fr_last_error().decode(), (name, L.fr_last_error())
        wk.sync()
        rows, bits = out.read(name)
        assert (rows.view(np.uint32) == R.CANARY).all() and (bits == R.CANARY).all(), "a refused call wrote its outputs"
        out.free()
        d_q.free()
        wk.close()
    finally:
        ctx.close()


def check_companion(fr):
    """libfleetrec_retrieve_lp.so (companion.check_companion): two scan instantiations (KP = 64 / 256; dim is a run-time bound) and the one image kernel,
    which builds and patches.  No VGPR cap: the scan holds a query tile and two row tiles in registers and runs one or two workgroups per CU by its LDS."""
    import companion
    companion.check_companion(fr, LP_LIB, ["fr_retrieve_lp_image_launch", "fr_retrieve_lp_scan_launch"], {"retrieve_lp_scan_kernel": 2, "retrieve_lp_image_kernel": 1},
                              "retrieve_lp_", (fr.LIB_PATH, R.RANK_LIB, T.RETRIEVE_LIB), max_vgprs=None)

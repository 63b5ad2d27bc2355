"""Probed bf16 retrieval over the table image (fr_worker_retrieve_probed_image_device / fr_worker_retrieve_probed_image): the checks, stated once in numpy
and parameterised by device (tests/test_cpu_retrieve_probed_lp.py, device = -1, and tests/test_gpu_retrieve_probed_lp.py).  The reference is the contract in
numpy: tests/retrieve_probed.py's reference over both operands rounded to bf16 -- the probed call's candidates, float64 scores of the rounded operands."""
import os

import numpy as np

import rank_topk as R
import retrieve as T
import retrieve_lp as LP
import retrieve_probed as P

CPU = T.CPU
PROBE_LP_LIB = os.path.join(R.ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_retrieve_probe_lp.so")
# "A": retrieve_probed.OFF -- no list starts on an image tile, lists 3 | 4 and 5 | 6 share a tile, the long list splits at row 1157, mid-tile, the table's
# last tile is partial.  "B": one whole tile; a list from a tile's first row to a tile's last row; an empty list; a list that starts on a tile and splits
# at 2080, a tile boundary too (an off-by-one scans a tile too many or too few); the ids of retrieve_probed.probe_rows are mapped onto its four lists.
PARTS = {"A": (P.OFF, np.arange(P.N_LISTS, dtype=np.int32)), "B": (np.array([0, 32, 1056, 1056, T.ROWS], np.int64), np.array([3, 1, 3, 0, 1, 2, 0], np.int32))}
# (dim, k, n_q, n_probe, kind, partition): a pad inside the only step, in the second half, a step and a half, the maximum; the kinds of retrieve_probed.EXACT
EXACT = [(4, 1, 1, 1, "mixed", "A"), (12, 3, 33, 5, "common", "A"), (128, 64, 33, 8, "common", "A"), (4, 256, 33, 8, "common", "B"), (24, 64, 1, 5, "short", "A"),
         (128, 256, 1, 8, "mixed", "A"), (12, 3, 7, 1, "distinct", "A"), (128, 1, 33, 5, "common", "B"), (24, 256, 33, 8, "common", "A"), (24, 64, 1, 1, "long", "B"),
         (128, 3, 1, 2, "long", "A"), (12, 64, 4, 1, "distinct", "B"), (4, 3, 1, 2, "long", "B")]


def probed_image(fr, ctx, wk, Q, probe, k, host=False, what="", expect=None):
    """one probed image retrieval over table 0 + sync -> (rows, score bits); the device form's outputs sit between canaries; expect: the sync's status"""
    Q, probe = np.ascontiguousarray(Q, np.float32), np.ascontiguousarray(probe, np.int32)
    if host:
        rows, sc = wk.retrieve_probed_image(0, Q, probe, k)
        return rows, sc.view(np.uint32)
    d_q, d_p, out = fr.DeviceBuffer.from_numpy(ctx, Q), fr.DeviceBuffer.from_numpy(ctx, probe), R.Outputs(fr, ctx, len(Q), k)
    try:
        wk.retrieve_probed_image_device(0, len(Q), d_q, probe.shape[1], d_p, k, out.p_idx, out.p_sc)
        assert R.status_of(fr, wk.sync) == (fr.FR_OK if expect is None else expect), what
        return out.read(what)
    finally:
        for b in (out, d_q, d_p):
            b.free()


def case(fr, device, Tab, Q, probe, k, off=P.OFF, host=False, what="", expect=None):
    """table 0 <- Tab, the partition, the image, one call -> its result, checked against the reference; expect: the sync's status when it is not FR_OK (a clean call follows)"""
    m, ctx = T.context(fr, device, Tab.shape[1])
    try:
        ctx.upload_table(0, Tab)
        ctx.set_retrieve_lists(0, off)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        got = probed_image(fr, ctx, wk, Q, probe, k, host, what, expect)
        if expect is not None:
            R.assert_same(probed_image(fr, ctx, wk, Q, np.where(probe < len(off) - 1, probe, -1), k, host, what), got, "a clean call afterwards")
        wk.close()
    finally:
        ctx.close()
    with np.errstate(invalid="ignore"):
        R.assert_same(got, P.reference(LP.bf16(Q), LP.bf16(Tab), probe, k, off), what)
    return got


def exact_case(fr, device, dim, k, n_q, n_probe, kind, part):
    """integers in [-4, 4] and a few +-257 / +-259 (bf16: 256 and 260 -- an fp32 scan and a truncating conversion both miss): every fp32 sum is exact in any order"""
    rng = np.random.default_rng(7600 + dim + k + n_probe)
    Tab, Q = rng.integers(-4, 5, (T.ROWS, dim)).astype(np.float32), rng.integers(-4, 5, (n_q, dim)).astype(np.float32)
    Tab[4, 0], Tab[1157, dim - 1], Tab[2080, 0], Tab[1055, dim - 1], Tab[T.ROWS - 1, 1] = 259, -257, -259, 257, 257
    Q[0, 0], Q[-1, dim - 1], Q[n_q // 2, 1] = 259, -259, 257
    off, remap = PARTS[part]
    probe = P.probe_rows(kind, n_q, n_probe, rng)
    probe = np.where(probe < 0, -1, remap[np.maximum(probe, 0)]).astype(np.int32)
    return case(fr, device, Tab, Q, probe, k, off, host=(k + n_probe) % 2 == 0, what=str((dim, k, n_q, n_probe, kind, part)))


def ties_case(fr, device, k):
    """a table of ones, ids in descending order: the k lowest rows of the union, in order"""
    got = case(fr, device, np.ones((T.ROWS, 4), np.float32), np.ones((2, 4), np.float32), np.array([[6, 4, 2, 0, -1]] * 2, np.int32), k, what="ties")
    union = np.concatenate([np.arange(P.OFF[l], P.OFF[l + 1]) for l in (0, 2, 4, 6)])
    assert np.array_equal(got[0], np.stack([union[:k]] * 2))
    return got


def adversarial_case(fr, device, dim, k):
    """retrieve_lp.adversarial_case's bf16-exact ramp (row 64 a + b holds (a, 1, b)) inside the long list: ascending with the row, descending, all equal"""
    Tab, Q = np.zeros((T.ROWS, dim), np.float32), np.zeros((3, dim), np.float32)
    Tab[:, 0], Tab[:, 1], Tab[:, 2] = np.arange(T.ROWS) // 64 - 24, 1, np.arange(T.ROWS) % 64
    Q[0, 0], Q[0, 2], Q[2, 1] = 64, 1, 1
    Q[1] = -Q[0]
    return case(fr, device, Tab, Q, np.full((3, 1), P.LONG, np.int32), k, what="adversarial order, dim %d, k %d" % (dim, k))


def check_rounded(fr, device, dim):
    """hash-filled rows, every query probes all seven lists in shuffled order: fr_worker_retrieve_image_device over [4, ROWS), bit for bit, on the same back-end"""
    rng = np.random.default_rng(7700 + dim)
    Q = rng.uniform(-1, 1, (80, dim)).astype(np.float32)
    probe = np.stack([rng.permutation(P.N_LISTS) for _ in range(len(Q))]).astype(np.int32)
    m, ctx = T.context(fr, device, dim)
    try:
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.set_retrieve_lists(0, P.OFF)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        got = probed_image(fr, ctx, wk, Q, probe, 64, what="rounded")
        want = LP.retrieve(fr, ctx, wk, Q, 64, int(P.OFF[0]), int(P.OFF[-1] - P.OFF[0]), what="rounded, image call")
        wk.close()
    finally:
        ctx.close()
    R.assert_same(got, want, "rounded data against the image call, dim %d" % dim)


def check_special(fr, device):
    """retrieve_probed.check_special's table through the image path: NaN, +-inf, +0, -0 and mixed-zero rows under a positive and a negative query; the
    one-row NaN list 3 in front of a NaN row of list 5; k = 256 > the union's 135 rows: the NaN rows before the padding, and the -0 score delivered"""
    rng = np.random.default_rng(6900)
    Tab = rng.integers(-4, 5, (T.ROWS, 4)).astype(np.float32)
    l0, l3, l5 = int(P.OFF[0]), int(P.OFF[3]), int(P.OFF[5])
    Tab[l3], Tab[l5 + 2], Tab[l0 + 7] = np.nan, np.nan, np.nan
    Tab[l0 + 20], Tab[l0 + 21], Tab[l0 + 30], Tab[l0 + 31], Tab[l0 + 32] = (np.inf, 1, 1, 1), (-np.inf, 1, 1, 1), 0.0, -0.0, (0.0, -0.0, 0.0, -0.0)
    Q = np.array([[1, 2, 1, 3], [-1, -2, -1, -3]], np.float32)
    probe = np.array([[5, 3, 0], [0, 5, 3]], np.int32)
    got = case(fr, device, Tab, Q, probe, 256, what="special values")
    assert list(got[0][0, 132:136]) == [l0 + 7, l3, l5 + 2, -1] and got[0][0, 0] == l0 + 20 and (got[1][:, 132:135] == T.QNAN).all()
    for q, minus_zero_row in ((0, l0 + 31), (1, l0 + 30)):
        assert got[1][q][list(got[0][q]).index(minus_zero_row)] == 0x80000000 and (got[1][q] == 0).any()


def check_composition(fr, device):
    """both images, the coarse image call over the centroids writing the probe buffer, a row update inside list 4, the probed image call -- no sync in between"""
    rng = np.random.default_rng(7800)
    dim, n_q, n_probe, k, new_row = 32, 5, 3, 16, 2000
    Tab, Cen = rng.integers(-4, 5, (T.ROWS, dim)).astype(np.float32), rng.integers(-4, 5, (16, dim)).astype(np.float32)
    Tab[1930, 3], Cen[P.COMMON] = 259, 4
    Q = rng.integers(1, 5, (n_q, dim)).astype(np.float32)
    ctx = fr.Context(T.model(fr, dim, extra_dim=dim), device=device)
    try:
        ctx.upload_table(0, Tab)
        ctx.upload_table(1, Cen)
        ctx.set_retrieve_lists(0, P.OFF)
        ctx.set_retrieve_image(1)
        ctx.set_retrieve_image(0)
        wk = fr.Worker(ctx, 16)
        bufs = [fr.DeviceBuffer.from_numpy(ctx, a) for a in (Q, np.full((n_q, n_probe), -7, np.int32), np.array([new_row], np.int32), np.full((1, dim), 100, np.float32))]
        d_q, d_p, d_id, d_row = bufs
        out = R.Outputs(fr, ctx, n_q, k)
        wk.retrieve_image_device(1, 0, P.N_LISTS, n_q, d_q, n_probe, d_p, None)
        wk.update_rows(0, 1, d_id, d_row)
        wk.retrieve_probed_image_device(0, n_q, d_q, n_probe, d_p, k, out.p_idx, out.p_sc)
        wk.sync()
        got = out.read("composition")
        for b in bufs + [out]:
            b.free()
        wk.close()
    finally:
        ctx.close()
    Tab[new_row] = 100
    coarse = T.reference(T.scores64(Q, Cen[:P.N_LISTS]), 0, n_probe)[0]
    want = P.reference(Q, LP.bf16(Tab), coarse, k)
    assert (coarse[:, 0] == P.COMMON).all() and (want[0][:, 0] == new_row).all()
    R.assert_same(got, want, "composition")


# name -> (what the context has: lists, image, stale; the arguments that differ from a good call; the status; a word of the error text)
REFUSALS = {
    "no image": (dict(image=False), {}, "STATE", "no retrieval image"), "stale image": (dict(stale=True), {}, "STATE", "stale"),
    "no partition": (dict(lists=False), {}, "STATE", "no list partition"), "NULL probe": ({}, dict(p=None), "INVALID", "probe"),
    "k 257": ({}, dict(k=257), "INVALID", "k = 257"), "n_probe 257": ({}, dict(n_probe=257), "INVALID", "n_probe"),
    "ranking bound": ({}, dict(n_q=65536, n_probe=256, k=256), "INVALID", "2^24"),
}


def check_refusal(fr, device, name):
    """status, the text in fr_last_error, and both outputs untouched behind a following sync"""
    make, bad, status, word = REFUSALS[name]
    ctx = fr.Context(T.model(fr, 8), device=device)
    try:
        L = fr.lib()
        if make.get("lists", True):
            ctx.set_retrieve_lists(0, np.array([0, 10, 30], np.int64))
        if make.get("image", True):
            ctx.set_retrieve_image(0)
        if make.get("stale"):
            ctx.upload_table(0, np.ones((1, 8), np.float32), 5)
        wk = fr.Worker(ctx, 16)
        d_q, d_p, out = fr.DeviceBuffer.from_numpy(ctx, np.ones((2, 8), np.float32)), fr.DeviceBuffer.from_numpy(ctx, np.zeros((2, 2), np.int32)), R.Outputs(fr, ctx, 2, 4)
        a = dict(n_q=2, n_probe=2, p=d_p.ptr, k=4)
        a.update(bad)
        for entry in (L.fr_worker_retrieve_probed_image_device, L.fr_worker_retrieve_probed_image):
            got = entry(wk._h, 0, a["n_q"], d_q.ptr, a["n_probe"], a["p"], a["k"], out.p_idx, out.p_sc)
            assert got == getattr(fr, "FR_ERR_" + status), (name, got)
            assert word in L.fr_last_error().decode(), (name, L.fr_last_error())
        wk.sync()
        rows, bits = out.read(name)
        assert (rows.view(np.uint32) == R.CANARY).all() and (bits == R.CANARY).all(), "a refused call wrote its outputs"
        for b in (out, d_q, d_p):
            b.free()
        wk.close()
    finally:
        ctx.close()


def check_index_range(fr, device):
    """an id >= n_lists: FR_ERR_INDEX_RANGE at the sync, the id scanned as no list, every query's result what the valid ids give; a clean call afterwards"""
    rng = np.random.default_rng(7900)
    Tab, Q = rng.integers(-4, 5, (T.ROWS, 4)).astype(np.float32), rng.integers(-4, 5, (3, 4)).astype(np.float32)
    case(fr, device, Tab, Q, np.array([[0, 3], [P.N_LISTS, 5], [6, 2 ** 31 - 1]], np.int32), 8, what="id out of range", expect=fr.FR_ERR_INDEX_RANGE)


def check_companion(fr):
    """its one launcher, the two scan instantiations (KP = 64 / 256), no spill, no private segment, $ORIGIN; 256 VGPRs: what two workgroups per CU leave a wave"""
    import companion
    companion.check_companion(fr, PROBE_LP_LIB, ["fr_retrieve_probe_lp_scan_launch"], {"retrieve_probe_lp_scan_kernel": 2}, "retrieve_probe_lp_",
                              (fr.LIB_PATH, R.RANK_LIB, T.RETRIEVE_LIB, LP.LP_LIB, P.PROBE_LIB), max_vgprs=256)


# test id -> (check, its arguments behind (fr, device)).  A check that returns its result is run on the device AND on the CPU back-end by the GPU module,
# which compares the two bit for bit.
CHECKS = {"exact %d-%d-%d-%d-%s-%s" % c: (exact_case, c) for c in EXACT}
CHECKS.update({"ties, k %d" % k: (ties_case, (k,)) for k in (64, 256)})
CHECKS.update({"adversarial order, dim %d, k %d" % a: (adversarial_case, a) for a in LP.ADVERSARIAL})
CHECKS.update({"rounded against the image call, dim %d" % d: (check_rounded, (d,)) for d in (32, 128)})
CHECKS.update({"special values": (check_special, ()), "composition and stream order": (check_composition, ()), "id out of range": (check_index_range, ())})
CHECKS.update({"refusal: " + name: (check_refusal, (name,)) for name in REFUSALS})

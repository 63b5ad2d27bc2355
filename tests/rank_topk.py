"""Segmented top-K ranking of scores (fr_worker_topk_device / fr_worker_topk): the checks, stated once in numpy and parameterised by device; the
tests are tests/test_cpu_rank_topk.py (device = -1) and tests/test_gpu_rank_topk.py.  The reference is the contract in numpy: the key of every
score's bits, np.lexsort((position, 0xffffffff - key)) per segment, padded with -1 / -inf.  Every comparison is np.array_equal on int32 and on
uint32 views of the scores; there is no tolerance anywhere."""
import ctypes
import os
import socket
import subprocess
import time

import numpy as np

CPU = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "host")
RANK_LIB = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_rank.so")
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 16384, 16385, 70001)
KS = (1, 2, 7, 64, 255, 256)
CLASSES = ("random_bits", "all_equal", "five_values", "zeros", "infs", "denormals", "ascending", "descending")
NEG_INF = np.uint32(0xff800000)
CANARY = 0x5a5a5a5a
GUARD = 64   # canary words on either side of an output array


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------

def keys(bits):
    u = np.asarray(bits, np.uint32)
    key = np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[(u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)] = 0
    return key


def ranked(bits):
    """positions of one segment in rank order"""
    key = keys(bits).astype(np.int64)
    return np.lexsort((np.arange(len(key)), 0xffffffff - key)).astype(np.int32)


def reference(bits, k, offsets=None):
    """-> (idx int32 [n_seg][k], scores uint32 [n_seg][k], malformed bool [n_seg])"""
    bits = np.asarray(bits, np.uint32)
    n = len(bits)
    off = np.array([0, n], np.int64) if offsets is None else np.asarray(offsets, np.int64)
    n_seg = len(off) - 1
    idx, sc, bad = np.full((n_seg, k), -1, np.int32), np.full((n_seg, k), NEG_INF, np.uint32), np.zeros(n_seg, bool)
    for s in range(n_seg):
        a, b = int(off[s]), int(off[s + 1])
        if a < 0 or b < a or b > n:
            bad[s] = True
            continue
        order = ranked(bits[a:b])[:k]
        idx[s, :len(order)] = order
        sc[s, :len(order)] = bits[a:b][order]
    return idx, sc, bad


def values(cls, n, rng):
    """n score bit patterns of a value class"""
    if cls == "random_bits":      # every fp32 class, NaNs of both signs included
        return rng.integers(0, 2 ** 32, size=n, dtype=np.uint32)
    if cls == "all_equal":        # position order alone decides
        return np.full(n, np.float32(0.625).view(np.uint32), np.uint32)
    if cls == "five_values":
        return np.array([-2.5, 0.0, 1.0, 1.0000001, 3e38], np.float32).view(np.uint32)[rng.integers(0, 5, size=n)]
    if cls == "zeros":            # +0 ranks above -0
        return np.array([0x00000000, 0x80000000], np.uint32)[rng.integers(0, 2, size=n)]
    if cls == "infs":
        return np.array([0x7f800000, 0xff800000, 0x3f800000, 0x7fc00000, 0xffc00001], np.uint32)[rng.integers(0, 5, size=n)]
    if cls == "denormals":
        return (rng.integers(1, 2 ** 23, size=n, dtype=np.uint32) | (rng.integers(0, 2, size=n, dtype=np.uint32) << np.uint32(31))).astype(np.uint32)
    ramp = np.arange(n, dtype=np.float32) - np.float32(n // 2)
    return (ramp if cls == "ascending" else ramp[::-1].copy()).view(np.uint32)


# ---- one call, its outputs between canaries -----------------------------------------------------------------------------------------------------

class Outputs:
    """[n_seg][k] int32 positions and float32 scores in device memory, each between two canary regions"""

    def __init__(self, fr, ctx, n_seg, k, with_scores=True):
        self.fr, self.count = fr, n_seg * k
        self.shape = (n_seg, k)
        guard = np.full(2 * GUARD + self.count, CANARY, np.uint32)
        self.d_idx = fr.DeviceBuffer.from_numpy(ctx, guard)
        self.d_sc = fr.DeviceBuffer.from_numpy(ctx, guard)
        self.with_scores = with_scores
        self.p_idx = self.d_idx.ptr.value + 4 * GUARD
        self.p_sc = self.d_sc.ptr.value + 4 * GUARD if with_scores else None

    def read(self, what=""):
        """-> (idx, score bits); the canaries are checked, and so is the whole score array when no scores were asked for"""
        i = self.d_idx.download(np.uint32, 2 * GUARD + self.count)
        s = self.d_sc.download(np.uint32, 2 * GUARD + self.count)
        for name, a in (("idx", i), ("scores", s)):
            assert (a[:GUARD] == CANARY).all() and (a[GUARD + self.count:] == CANARY).all(), "%s: a canary around %s was written" % (what, name)
        if not self.with_scores:
            assert (s == CANARY).all(), "%s: scores were written although d_top_scores was NULL" % what
        return i[GUARD:GUARD + self.count].view(np.int32).reshape(self.shape), s[GUARD:GUARD + self.count].reshape(self.shape)

    def free(self):
        self.d_idx.free()
        self.d_sc.free()


def rank(fr, ctx, wk, bits, k, offsets=None, with_scores=True, d_scores=None, expect=None, what=""):
    """One fr_worker_topk_device + sync over `bits` -> (idx, score bits); expect = a status the sync must return instead of FR_OK."""
    bits = np.ascontiguousarray(bits, np.uint32)
    n_seg = 1 if offsets is None else len(offsets) - 1
    own = d_scores is None
    if own:
        d_scores = fr.DeviceBuffer.from_numpy(ctx, bits if len(bits) else np.zeros(1, np.uint32))
    d_off = None if offsets is None else fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(offsets, np.int32))
    out = Outputs(fr, ctx, n_seg, k, with_scores)
    try:
        wk.topk_device(len(bits), d_scores, k, out.p_idx, out.p_sc, d_off, n_seg)
        got = status_of(fr, wk.sync)
        assert got == (fr.FR_OK if expect is None else expect), "%s: sync returned %d" % (what, got)
        return out.read(what)
    finally:
        out.free()
        if d_off is not None:
            d_off.free()
        if own:
            d_scores.free()


def status_of(fr, fn):
    try:
        fn()
    except fr.FleetRecError as e:
        return e.status
    return fr.FR_OK


def assert_same(got, want, what):
    gi, gs = got
    wi, ws = want[0], want[1]
    assert np.array_equal(gi, wi), "%s: %d of %d positions differ" % (what, int((gi != wi).sum()), wi.size)
    assert np.array_equal(gs, ws), "%s: %d of %d score bit patterns differ" % (what, int((gs != ws).sum()), ws.size)


def small_context(fr, device, max_rows=2000):
    m = fr.Model.builtin(fr.MODEL_A).clone(row_scale=0.001, max_rows=max_rows)
    ctx = fr.Context(m, device=device)
    ctx.fill_tables(fr.FILL_HASH, 7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
    return m, ctx


# ---- 1. values ---------------------------------------------------------------------------------------------------------------------------------

def check_values(fr, device, cls):
    """Every length x every k of one value class, as one segment in the NULL-offsets form (length 0: an empty segment of a one-score array), then all
    the lengths at once as the segments of one call, per k.  The rank order of a (class, length) is computed once and shared by the ks."""
    rng = np.random.default_rng(5100 + CLASSES.index(cls))
    m, ctx = small_context(fr, device, 200)
    try:
        wk = fr.Worker(ctx, 16)
        parts = [values(cls, n, rng) for n in LENGTHS]
        orders = [ranked(p) for p in parts]

        def want(i, k):
            idx, sc = np.full(k, -1, np.int32), np.full(k, NEG_INF, np.uint32)
            o = orders[i][:k]
            idx[:len(o)], sc[:len(o)] = o, parts[i][o]
            return idx, sc

        for i, n in enumerate(LENGTHS):
            bits = parts[i] if n else values(cls, 1, rng)
            d_scores = fr.DeviceBuffer.from_numpy(ctx, bits)
            try:
                for k in KS:
                    what = "%s, length %d, k %d" % (cls, n, k)
                    got = rank(fr, ctx, wk, bits, k, None if n else [0, 0], d_scores=d_scores, what=what)
                    wi, ws = want(i, k)
                    assert_same(got, (wi[None, :], ws[None, :]), what)
            finally:
                d_scores.free()
        allbits = np.concatenate(parts)
        offsets = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int32)
        d_scores = fr.DeviceBuffer.from_numpy(ctx, allbits)
        try:
            for k in KS:
                what = "%s, every length as a segment, k %d" % (cls, k)
                got = rank(fr, ctx, wk, allbits, k, offsets, d_scores=d_scores, what=what)
                ws = [want(i, k) for i in range(len(LENGTHS))]
                assert_same(got, (np.stack([w[0] for w in ws]), np.stack([w[1] for w in ws])), what)
        finally:
            d_scores.free()
        wk.close()
    finally:
        ctx.close()


# ---- 2. segments ---------------------------------------------------------------------------------------------------------------------------------

def check_segments(fr, device):
    """n_seg of 1, 3, 257 and 1000; empty segments among full ones; offsets that start above 0 and end below n; 1000 segments of lengths 0 .. 9; the
    NULL-offsets form; indices only (d_top_scores NULL)."""
    rng = np.random.default_rng(5200)
    m, ctx = small_context(fr, device, 200)
    try:
        wk = fr.Worker(ctx, 16)
        cases = []
        for n_seg, n in ((1, 5000), (3, 40000), (257, 30000), (1000, 100000)):
            cuts = np.sort(rng.integers(0, n + 1, size=n_seg - 1)) if n_seg > 1 else np.zeros(0, np.int64)
            cases.append(("%d random segments of %d" % (n_seg, n), n, np.concatenate([[0], cuts, [n]])))
        cases.append(("empty segments among full ones", 9000, np.array([0, 0, 4096, 4096, 4096, 4353, 9000, 9000])))
        cases.append(("offsets inside the array", 20000, np.array([37, 1000, 1000, 18001, 19990])))
        cases.append(("1000 segments of 0 .. 9", 4500, np.concatenate([[0], np.cumsum(np.arange(1000) % 10)])))
        cases.append(("one long segment beside short ones", 60000, np.array([0, 3, 50003, 50003, 60000])))
        cases.append(("n + 1 segments", 7, np.array([0, 0, 1, 2, 3, 5, 6, 7])))
        for what, n, off in cases:
            bits = values("random_bits", n, rng) if "1000 seg" not in what else values("five_values", n, rng)
            for k in (1, 7, 256):
                assert_same(rank(fr, ctx, wk, bits, k, off, what=what), reference(bits, k, off), "%s, k %d" % (what, k))
            gi, gs = rank(fr, ctx, wk, bits, 7, off, with_scores=False, what=what)
            assert np.array_equal(gi, reference(bits, 7, off)[0]), what + ": indices only"
        for n in (1, 255, 5000, 16384, 16385):
            bits = values("random_bits", n, rng)
            assert_same(rank(fr, ctx, wk, bits, 64, None, what="NULL offsets"), reference(bits, 64), "NULL offsets, n %d" % n)
        wk.close()
    finally:
        ctx.close()


def check_long_segment(fr, device):
    """A lone segment past every single-launch size (2^20 + 3 scores: 65 units, two merge levels), beside a second call of 2^18 that reuses the
    scratch; five distinct values, so position order decides among 200000 equal keys."""
    rng = np.random.default_rng(5300)
    m, ctx = small_context(fr, device, 200)
    try:
        wk = fr.Worker(ctx, 16)
        for n, cls in ((2 ** 20 + 3, "five_values"), (2 ** 18, "random_bits")):
            bits = values(cls, n, rng)
            assert_same(rank(fr, ctx, wk, bits, 256, None, what="lone long segment"), reference(bits, 256), "lone segment of %d, k 256" % n)
        bits = values("random_bits", 300000, rng)
        off = np.array([5, 150000, 150001, 299999])
        assert_same(rank(fr, ctx, wk, bits, 33, off, what="two long segments"), reference(bits, 33, off), "two long segments, k 33")
        wk.close()
    finally:
        ctx.close()


# ---- 3. malformed offsets ------------------------------------------------------------------------------------------------------------------------

MALFORMED = {
    "start below 0": [0, 100, -5, 300, 700, 1000],                 # segment 1 ends below its start, segment 2 starts below 0
    "end below start": [0, 400, 200, 650, 1000],                   # segment 1
    "end above n": [0, 100, 1001, 1001, 600, 1000],                # segments 1 (end > n), 2 (start and end > n) and 3 (end < start)
    "far outside": [0, 500, 2 ** 31 - 1, -2 ** 31, 20, 1000],      # the int32 extremes
    "every class": [0, 100, -5, 200, 150, 400, 2000, 600, 1000],
}


def check_malformed(fr, device):
    """One malformed segment of each class among clean ones: FR_ERR_INDEX_RANGE at sync, the clean segments exact, the malformed ones empty (the
    reference ranks them as empty), and a clean call afterwards succeeds -- also past 16384 scores, where the long-segment kernels check again."""
    rng = np.random.default_rng(5400)
    m, ctx = small_context(fr, device, 200)
    try:
        wk = fr.Worker(ctx, 16)
        bits = values("random_bits", 1000, rng)
        for what, off in MALFORMED.items():
            want = reference(bits, 9, off)
            assert want[2].any() and not want[2].all()
            got = rank(fr, ctx, wk, bits, 9, off, expect=fr.FR_ERR_INDEX_RANGE, what=what)
            assert_same(got, want, what)
            assert (got[0][want[2]] == -1).all() and (got[1][want[2]] == NEG_INF).all()
            assert_same(rank(fr, ctx, wk, bits, 9, [0, 500, 1000], what="clean call after " + what), reference(bits, 9, [0, 500, 1000]), "clean call after " + what)
        big = values("random_bits", 90000, rng)
        off = [0, 40000, 90001, 39000, 89000, 90000, -1, 90000]    # long clean segments (one overlapping another) among malformed ones
        want = reference(big, 17, off)
        assert list(want[2]) == [False, True, True, False, False, True, True]
        assert_same(rank(fr, ctx, wk, big, 17, off, expect=fr.FR_ERR_INDEX_RANGE, what="long segments"), want, "malformed among long segments")
        assert_same(rank(fr, ctx, wk, big, 17, None, what="clean long call"), reference(big, 17), "clean long call afterwards")
        wk.close()
    finally:
        ctx.close()


# ---- 4. stream order -------------------------------------------------------------------------------------------------------------------------------

def check_stream_order(fr, device, group):
    """Four batches of 256 pushed with push_device into one contiguous 1024-float score buffer, then topk_device with 8 segments of 128, no sync in
    between: group 64 leaves the batches queued for a fused launch, group 1 in the stage pipeline.  Then the same after submit_pooled_device (one
    batch, two segments) and after four push_pooled_device.  The result equals the reference applied to the scores of a plain synchronised run."""
    rng = np.random.default_rng(5500 + group)
    m, ctx = small_context(fr, device)
    try:
        ctx.set_stream_group(group)
        B, NB, K = 256, 4, 10
        ranges = m.index_ranges()
        wk = fr.Worker(ctx, B)
        d_sc = fr.DeviceBuffer(ctx, NB * B * 4)
        part = lambda i: d_sc.ptr.value + i * B * 4
        off8 = np.arange(0, NB * B + 1, 128, dtype=np.int32)
        d_off8, d_off2 = fr.DeviceBuffer.from_numpy(ctx, off8), fr.DeviceBuffer.from_numpy(ctx, off8[:3])
        zero = np.zeros(NB * B, np.uint32)

        def ranked_run(push, n_batches, d_off, n_seg, what):
            d_sc.upload(zero)
            for i in range(n_batches):          # the plain synchronised run
                push(i)
                wk.sync()
            plain = d_sc.download(np.uint32, n_batches * B)
            named = wk.last_kernel()
            assert len(set(plain.tolist())) > B // 2, what + ": the scores do not differ"
            d_sc.upload(zero)
            out = Outputs(fr, ctx, n_seg, K)
            try:
                for i in range(n_batches):      # the sequence under test: no sync before the end
                    push(i)
                wk.topk_device(n_batches * B, d_sc, K, out.p_idx, out.p_sc, d_off, n_seg)
                wk.sync()
                assert_same(out.read(what), reference(plain, K, off8[:n_seg + 1]), what)
                assert np.array_equal(d_sc.download(np.uint32, n_batches * B), plain)
                assert wk.last_kernel() == named and "rank" not in named, (named, wk.last_kernel())   # it keeps naming the last batch's kernel
            finally:
                out.free()

        idx = [(rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32) for _ in range(NB)]
        d_idx = [fr.DeviceBuffer.from_numpy(ctx, a) for a in idx]
        ranked_run(lambda i: wk.push_device(B, d_idx[i], None, part(i)), NB, d_off8, 8, "group %d: four pushes" % group)
        # pooled lookups: two slots per column, some empty
        hots = np.full(m.idx_cols, 2, np.int32)
        wk.close()
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, B)
        pidx = []
        for _ in range(NB):
            a = (rng.random((B, len(ranges), 2)) * ranges[None, :, None]).astype(np.int32)
            a[rng.random(a.shape) < 0.2] = -1
            pidx.append(a.reshape(B, -1))
        d_pidx = [fr.DeviceBuffer.from_numpy(ctx, a) for a in pidx]
        ranked_run(lambda i: wk.submit_pooled_device(B, d_pidx[i], None, part(i)), 1, d_off2, 2, "group %d: submit_pooled_device" % group)
        ranked_run(lambda i: wk.push_pooled_device(B, d_pidx[i], None, part(i)), NB, d_off8, 8, "group %d: four pooled pushes" % group)
        for b in d_idx + d_pidx + [d_sc, d_off8, d_off2]:
            b.free()
        wk.close()
    finally:
        ctx.close()


# ---- 5. the host form ------------------------------------------------------------------------------------------------------------------------------

def host_form_results(fr, device):
    """infer_topk after each of the four host submit forms -> the list of (what, scores of the plain infer, (idx, score bits) of the ranked one)"""
    rng = np.random.default_rng(5600)
    m, ctx = small_context(fr, device)
    out = []
    try:
        B, K = 200, 12
        off = np.array([0, 50, 50, 130, 200], np.int32)
        ranges = m.index_ranges()
        idx = (rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32)
        wk = fr.Worker(ctx, 256)
        plain = wk.infer(idx).view(np.uint32)
        gi, gs = wk.infer_topk(idx, K, off)
        out.append(("submit", plain, (gi, gs.view(np.uint32))))
        gi, gs = wk.infer_topk(idx, K)                      # NULL offsets: the whole batch
        out.append(("submit, one segment", plain, (gi, gs.view(np.uint32))))
        wk.close()
        hots = np.full(m.idx_cols, 2, np.int32)
        ctx.set_pooling(hots)
        wk = fr.Worker(ctx, 256)
        a = (rng.random((B, len(ranges), 2)) * ranges[None, :, None]).astype(np.int32)
        a[rng.random(a.shape) < 0.2] = -1
        pidx = a.reshape(B, -1)
        wts = rng.standard_normal(pidx.shape).astype(np.float32)
        plain = wk.infer_pooled(pidx).view(np.uint32)
        gi, gs = wk.infer_pooled_topk(pidx, K, off)
        out.append(("submit_pooled", plain, (gi, gs.view(np.uint32))))
        plain = wk.infer_pooled(pidx, weights=wts).view(np.uint32)
        gi, gs = wk.infer_pooled_topk(pidx, K, off, weights=wts)
        out.append(("submit_pooled_weighted", plain, (gi, gs.view(np.uint32))))
        c_off, c_ind, c_w = fr.bags_to_csr(pidx, hots, wts)
        plain = wk.infer_pooled_csr(c_off, c_ind).view(np.uint32)
        gi, gs = wk.infer_pooled_csr_topk(c_off, c_ind, K, off)
        out.append(("submit_pooled_csr", plain, (gi, gs.view(np.uint32))))
        # the staging grows: more segments x k than before
        off2 = np.arange(0, B + 1, 2, dtype=np.int32)
        plain = wk.infer_pooled(pidx).view(np.uint32)
        gi, gs = wk.infer_pooled_topk(pidx, 256, off2)
        out.append(("grown staging", plain, (gi, gs.view(np.uint32))))
        for what, plain, got in out:
            o = off2 if what == "grown staging" else (None if "one segment" in what else off)
            assert_same(got, reference(plain, got[0].shape[1], o), "host form after " + what)
        wk.close()
    finally:
        ctx.close()
    return out


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------------------------

def check_errors(fr, device):
    """Every FR_ERR_INVALID / FR_ERR_STATE case of the contract; nothing is enqueued on such an error: the outputs keep their canaries and a
    following sync is clean."""
    rng = np.random.default_rng(5700)
    m, ctx = small_context(fr, device)
    try:
        L = fr.lib()
        B = 64
        wk = fr.Worker(ctx, B)
        bits = values("random_bits", 100, rng)
        d_scores = fr.DeviceBuffer.from_numpy(ctx, bits)
        d_off = fr.DeviceBuffer.from_numpy(ctx, np.array([0, 50, 100], np.int32))
        out = Outputs(fr, ctx, 2, 4)
        h, ps = wk._h, d_scores.ptr

        def dev(n=100, scores=ps, n_seg=2, off=d_off.ptr, k=4, ti=out.p_idx, ts=out.p_sc):
            return L.fr_worker_topk_device(h, n, scores, n_seg, off, k, ti, ts)

        for bad in (dict(k=0), dict(k=-1), dict(k=257), dict(n=0), dict(n=-3), dict(n=2 ** 24 + 1), dict(n_seg=0), dict(n_seg=-1), dict(n_seg=102),
                    dict(scores=None), dict(ti=None)):
            assert dev(**bad) == fr.FR_ERR_INVALID, bad
        assert L.fr_worker_topk_device(None, 100, ps, 2, d_off.ptr, 4, out.p_idx, out.p_sc) == fr.FR_ERR_INVALID
        wk.sync()
        gi, gs = out.read("refused device calls")
        assert (gi.view(np.uint32) == CANARY).all() and (gs == CANARY).all(), "a refused call wrote its outputs"
        # the host form: no host-form batch in flight; wrong batch; arguments; a second ranking in flight
        hi, hs = np.full((2, 4), -7, np.int32), np.full((2, 4), 7.0, np.float32)
        off = np.array([0, 10, B], np.int32)
        pv = lambda a: a.ctypes.data_as(ctypes.c_void_p)

        def host(batch=B, n_seg=2, o=off, k=4, ti=hi, ts=hs):
            return L.fr_worker_topk(h, batch, n_seg, None if o is None else pv(o), k, None if ti is None else pv(ti), None if ts is None else pv(ts))

        assert host() == fr.FR_ERR_STATE                      # nothing submitted
        wk.topk_device(100, d_scores, 4, out.p_idx, out.p_sc, d_off, 2)
        assert host() == fr.FR_ERR_STATE                      # a device-form ranking is not a host-form batch
        wk.sync()
        ranges = m.index_ranges()
        idx = (rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32)
        plain = wk.infer(idx).view(np.uint32)
        assert host() == fr.FR_ERR_STATE                      # synchronised: no longer in flight
        wk.idx[:B] = idx
        wk.submit(B)
        for bad in (dict(k=0), dict(k=257), dict(batch=B - 1), dict(batch=0), dict(n_seg=0), dict(n_seg=B + 2), dict(ti=None)):
            assert host(**bad) == fr.FR_ERR_INVALID, bad
        assert L.fr_worker_topk(None, B, 2, pv(off), 4, pv(hi), pv(hs)) == fr.FR_ERR_INVALID
        assert host() == fr.FR_OK
        if device != CPU:                                     # (the CPU back-end has computed the first already)
            assert host() == fr.FR_ERR_STATE                  # one host-form ranking in flight per worker
        wk.sync()
        want = reference(plain, 4, off)
        assert np.array_equal(hi, want[0]) and np.array_equal(hs.view(np.uint32), want[1])
        assert host() == fr.FR_ERR_STATE                      # the sync ended the batch
        # host-fed batches queued in a block: flush first
        if device != CPU:
            sc_out = np.zeros(B, np.float32)
            wk.push_host(idx, None, sc_out)
            assert wk.host_pending()[0] == 1
            try:
                wk.topk_device(100, d_scores, 4, out.p_idx, out.p_sc, d_off, 2)
                raise AssertionError("a ranking beside a queued host-fed batch was accepted")
            except fr.FleetRecError as e:
                assert e.status == fr.FR_ERR_STATE and "flush first" in str(e), e
            wk.sync()
            assert np.isfinite(sc_out).all() and sc_out.any()   # the refused ranking left the host-fed batch to its sync (the fused kernel's scores)
        # after a sharded step the host form refuses
        for b in (d_scores, d_off):
            b.free()
        out.free()
        wk.close()
    finally:
        ctx.close()
    c0 = fr.Context(m, device=device, shard_rank=0, n_shards=2)
    try:
        w0 = fr.Worker(c0, 16)
        hi = np.zeros((1, 4), np.int32)
        assert fr.lib().fr_worker_topk(w0._h, 16, 1, None, 4, hi.ctypes.data_as(ctypes.c_void_p), None) == fr.FR_ERR_STATE
        w0.sync()
        w0.close()
    finally:
        c0.close()


# ---- 7. the server ---------------------------------------------------------------------------------------------------------------------------------

def _recv_exact(sk, n):
    buf = b""
    while len(buf) < n:
        part = sk.recv(n - len(buf))
        assert part, "the server closed the connection"
        buf += part
    return buf


def _connect(port, deadline):
    while True:
        try:
            return socket.create_connection(("127.0.0.1", port), timeout=60)
        except OSError:
            assert time.time() < deadline, "the server never listened on port %d" % port
            time.sleep(0.05)


def check_server(fr, device, free_port_block):
    """fleetrec_server --topk 4 --segments 2 --reply: a block's answer is 2 x 4 little-endian (int32 position, float32 score) pairs -- the
    reference applied to the library's own scores of the block; then --topk with --stream and with --shards is refused with a reason."""
    server = os.path.join(HOST, "fleetrec_server")
    if not os.path.exists(server):
        subprocess.check_call(["make", "-s", "-C", HOST])
    B, cap, K, S = 64, 200, 4, 2
    m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=cap)
    rng = np.random.default_rng(5800)
    ranges = m.index_ranges()
    blocks = [(rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32) for _ in range(2)]
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
        wk = fr.Worker(ctx, B)
        plain = [wk.infer(b).view(np.uint32) for b in blocks]
        wk.close()
    finally:
        ctx.close()
    common = ["--model", "A", "--batch", str(B), "--threads", "1", "--tables", "hash", "--weights", "uniform", "--row-cap", str(cap), "--device", str(device)]
    port = free_port_block(1)
    srv = subprocess.Popen([server] + common + ["--port", str(port), "--total", "2", "--reply", "--topk", str(K), "--segments", str(S)],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    try:
        sk = _connect(port, time.time() + 120)
        pair = np.dtype([("pos", "<i4"), ("score", "<u4")])
        for b, sc in zip(blocks, plain):
            sk.sendall(b.tobytes())
            got = np.frombuffer(_recv_exact(sk, S * K * 8), pair).reshape(S, K)
            want = reference(sc, K, [0, B // 2, B])
            assert np.array_equal(got["pos"], want[0]) and np.array_equal(got["score"], want[1])
        sk.close()
        out, _ = srv.communicate(timeout=120)
        assert srv.returncode == 0, out.decode()
    finally:
        if srv.poll() is None:
            srv.kill()
    for extra, word in ((["--stream"], "--stream"), (["--shards", "2"], "--shards"), (["--segments", "3"], "--segments")):
        r = subprocess.run([server] + common + ["--port", str(port), "--total", "1", "--reply", "--topk", str(K)] + extra, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode != 0 and b"--topk" in r.stdout and word.encode() in r.stdout, r.stdout.decode()


# ---- 8. the companion code object -------------------------------------------------------------------------------------------------------------------

def check_companion(fr):
    """libfleetrec_rank.so (companion.check_companion; its kernels keep a top-K heap in registers: no VGPR cap is stated for them)"""
    import companion
    companion.check_companion(fr, RANK_LIB, ["fr_rank_launch"], {"rank_parts_kernel": 1, "rank_merge_kernel": 1, "rank_segments_kernel": 2}, "rank_", (fr.LIB_PATH,), max_vgprs=None)

"""Request-form batches (fr_ctx_set_request_columns / fr_worker_expand_requests_device / fr_worker_submit_requests): the checks, stated once in
numpy and parameterised by device; the tests are tests/test_cpu_request_form.py (device = -1) and tests/test_gpu_request_form.py.  The reference
is the contract in numpy (expand): every word of a shared column from the row of the owning request, every other word from the candidate row.
Every comparison is np.array_equal on uint32 views; there is no tolerance anywhere -- the expansion moves words, and everything behind it is the
code that runs on host-expanded rows."""
import ctypes
import os
import subprocess
import time

import numpy as np

import rank_topk as R

CPU = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "host")
REQUEST_LIB = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_request.so")
BATCHES = (1, 63, 64, 65, 301, 4097)   # 4097: past whatever one workgroup covers, at every row width used here
CANARY = 0x5a5a5a5a
GUARD = 64   # canary words on either side of the output
SPECIAL = np.array([0xffffffff, 0x80000000, 0xfffffffe, 0x7fc00000, 0xffc00001, 0x7f800000, 0xff800000, 0x7fffffff, 0], np.uint32)   # -1, negatives, NaNs, infs


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------

def word_mask(shared, hots=None):
    """bool [W]: which words of a full row are the request's (hots: the pooled form's slots per column)"""
    sh = np.asarray(shared, bool)
    return sh if hots is None else np.repeat(sh, np.asarray(hots, np.int64))


def owners(off, batch, n_req):
    if off is None:
        return np.arange(batch) // (batch // n_req)
    return np.repeat(np.arange(n_req), np.diff(np.asarray(off, np.int64)))


def expand(req, cand, mask, off, n_req=None):
    """req [n_req][Rs] + cand [B][Rc] (any 4-byte dtype) -> full rows uint32 [B][W]; off: well-formed offsets, or None for the equal split"""
    mask = np.asarray(mask, bool)
    B = len(cand)
    n_req = len(req) if n_req is None else n_req
    out = np.empty((B, mask.size), np.uint32)
    out[:, ~mask] = np.ascontiguousarray(cand).view(np.uint32).reshape(B, int((~mask).sum()))
    out[:, mask] = np.ascontiguousarray(req).view(np.uint32).reshape(n_req, int(mask.sum()))[owners(off, B, n_req)]
    return out


def split(full, mask, off):
    """full rows [B][W] -> (req [n_req][Rs], cand [B][Rc]): the request row is the row of the request's first item (an empty request: zeros)"""
    mask = np.asarray(mask, bool)
    off = np.asarray(off, np.int64)
    first = np.minimum(off[:-1], len(full) - 1)
    req = full[first][:, mask].copy()
    req[np.diff(off) == 0] = 0
    return req, np.ascontiguousarray(full[:, ~mask])


def random_words(rng, shape):
    """random 32-bit patterns, one in eight of them a -1, another negative, a NaN or an infinity"""
    a = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint32)
    pick = rng.random(shape) < 0.125
    a[pick] = SPECIAL[rng.integers(0, len(SPECIAL), size=int(pick.sum()))]
    return a


def random_offsets(rng, batch, n_req):
    cuts = np.sort(rng.integers(0, batch + 1, size=n_req - 1)) if n_req > 1 else np.zeros(0, np.int64)
    return np.concatenate([[0], cuts, [batch]]).astype(np.int32)


# ---- models and contexts (all small) ------------------------------------------------------------------------------------------------------------

def model(fr, kind):
    if kind == "A":
        return fr.Model.builtin(fr.MODEL_A).clone(max_rows=200)
    if kind in ("C", "C_bank", "C_item"):
        mode = {"C": None, "C_bank": fr.INDEX_PER_BANK, "C_item": fr.INDEX_PER_ITEM}[kind]
        return fr.Model.builtin(fr.MODEL_C).clone(max_rows=200, index_mode=mode)
    assert kind == "narrow"
    return fr.Model.from_spec({"name": "narrow_rows", "tables": [{"dim": 8, "rows": 50}, {"dim": 8, "rows": 70}, {"dim": 16, "rows": 90}], "fc": [64, 32, 32]})


def context(fr, device, kind, precision=None):
    m = model(fr, kind)
    ctx = fr.Context(m, device=device)
    ctx.fill_tables(fr.FILL_HASH, 7)
    ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
    if precision:
        ctx.set_fc_precision(precision)
    return m, ctx


def masks(C):
    """first column only, last column only, alternating, all but one column"""
    first, last, alt, but = np.zeros(C, np.int32), np.zeros(C, np.int32), (np.arange(C) % 2 == 0).astype(np.int32), np.ones(C, np.int32)
    first[0], last[-1], but[C // 2] = 1, 1, 0
    return {"first": first, "last": last, "alternating": alt, "all but one": but}


def mixed_hots(C):
    return np.array([1, 3, 4, 64], np.int32)[np.arange(C) % 4]


# ---- one expansion, its output between canaries ----------------------------------------------------------------------------------------------------

def run_expand(fr, ctx, wk, form, req, cand, off, batch, n_req, row_words, shift=0, expect=None, what=""):
    """One fr_worker_expand_requests_device + sync -> uint32 [batch][row_words].  shift = 1: every array starts 4 bytes past a 16-byte boundary.
    expect: the status the sync must return instead of FR_OK.  The 64 canary words on either side of the output must be untouched."""
    bufs = []

    def dev(a):
        a = np.ascontiguousarray(a).view(np.uint32).reshape(-1)
        b = fr.DeviceBuffer.from_numpy(ctx, np.concatenate([np.zeros(4 + shift, np.uint32), a, np.zeros(1, np.uint32)]))
        bufs.append(b)
        return b.ptr.value + 4 * (4 + shift)

    count = batch * row_words
    d_out = fr.DeviceBuffer.from_numpy(ctx, np.full(2 * GUARD + shift + count, CANARY, np.uint32))
    bufs.append(d_out)
    try:
        p_req = dev(req)
        p_cand = dev(cand) if cand is not None and np.asarray(cand).size else (dev(np.zeros(1, np.uint32)) if cand is not None else None)
        p_off = dev(np.asarray(off, np.int32)) if off is not None else None
        wk.expand_requests_device(batch, n_req, p_req, p_cand, d_out.ptr.value + 4 * (GUARD + shift), form, p_off)
        got = R.status_of(fr, wk.sync)
        assert got == (fr.FR_OK if expect is None else expect), "%s: sync returned %d" % (what, got)
        a = d_out.download(np.uint32, 2 * GUARD + shift + count)
        assert (a[:GUARD + shift] == CANARY).all() and (a[GUARD + shift + count:] == CANARY).all(), "%s: a canary around the output was written" % what
        return a[GUARD + shift:GUARD + shift + count].reshape(batch, row_words)
    finally:
        for b in bufs:
            b.free()


def assert_rows(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d of %d words differ" % (what, int((got != want).sum()), want.size)


# ---- 1. words ------------------------------------------------------------------------------------------------------------------------------------

def check_words(fr, device, case):
    """Random 32-bit patterns through one form of one split, every batch size, aligned and 4 bytes off; against expand()."""
    rng = np.random.default_rng(6100 + sum(map(ord, case)))
    kind, form, hots = {"one-hot": ("A", fr.REQ_ONE_HOT, None), "one-hot narrow": ("narrow", fr.REQ_ONE_HOT, None), "pooled": ("A", fr.REQ_POOLED, "mixed"),
                        "pooled narrow": ("narrow", fr.REQ_POOLED, "mixed"), "dense": ("C", fr.REQ_DENSE, None), "per-item": ("C_item", fr.REQ_ONE_HOT, None),
                        "per-item dense": ("C_item", fr.REQ_DENSE, None), "per-bank": ("C_bank", fr.REQ_ONE_HOT, None)}[case]
    m, ctx = context(fr, device, kind)
    try:
        C = m.idx_cols
        if hots is not None:
            hots = mixed_hots(C)
            ctx.set_pooling(hots)
        wk = fr.Worker(ctx, max(BATCHES))
        splits = {"dense only": np.zeros(C, np.int32)} if kind == "C_item" else masks(C)
        if form == fr.REQ_DENSE and kind == "C":
            splits = {"first": masks(C)["first"]}
        for name, shared in splits.items():
            ctx.set_request_columns(shared, dense_shared=form == fr.REQ_DENSE or kind == "C_item")
            mask = np.ones(m.dense_len, bool) if form == fr.REQ_DENSE else word_mask(shared, hots)
            rs, rc, W = ctx.request_words(form)
            assert (rs, rc, W) == (int(mask.sum()), int((~mask).sum()), mask.size), (case, name, rs, rc, W)
            for n, B in enumerate(BATCHES):
                n_req = 1 + int(rng.integers(0, min(B, 40)))
                off = random_offsets(rng, B, n_req)
                req, cand = random_words(rng, (n_req, rs)), random_words(rng, (B, rc))
                what = "%s, %s, batch %d" % (case, name, B)
                got = run_expand(fr, ctx, wk, form, req, cand if rc else None, off, B, n_req, W, shift=n % 2, what=what)
                assert_rows(got, expand(req, cand, mask, off), what)
        wk.close()
    finally:
        ctx.close()


WORD_CASES = ("one-hot", "one-hot narrow", "pooled", "pooled narrow", "dense", "per-item", "per-item dense", "per-bank")


# ---- 2. segments ---------------------------------------------------------------------------------------------------------------------------------

def check_segments(fr, device):
    """n_req = 1, = batch, > batch; empty requests first, in the middle, last and in a row; one long request among single-item ones; NULL offsets."""
    rng = np.random.default_rng(6200)
    m, ctx = context(fr, device, "narrow")
    try:
        shared = np.array([1, 0, 1], np.int32)
        ctx.set_request_columns(shared)
        mask = word_mask(shared)
        B = 301
        wk = fr.Worker(ctx, 512)
        cases = {
            "one request": [0, B],
            "a request per item": np.arange(B + 1),
            "more requests than items": np.concatenate([[0], np.sort(rng.integers(0, B + 1, size=2 * B)), [B]]),
            "empty first": [0, 0, 100, B],
            "empty in the middle": [0, 100, 100, B],
            "empty last": [0, 100, B, B],
            "empty in a row": [0, 0, 0, 64, 64, 64, 64, 65, B, B, B],
            "one long request among single items": [0, 1, 2, B - 1, B],
        }
        for what, off in cases.items():
            off = np.asarray(off, np.int32)
            n_req = len(off) - 1
            req, cand = random_words(rng, (n_req, 2)), random_words(rng, (B, 1))
            assert_rows(run_expand(fr, ctx, wk, fr.REQ_ONE_HOT, req, cand, off, B, n_req, 3, what=what), expand(req, cand, mask, off), what)
        for batch, n_req in ((300, 1), (300, 300), (300, 20), (64, 4), (7, 7)):
            req, cand = random_words(rng, (n_req, 2)), random_words(rng, (batch, 1))
            what = "NULL offsets, %d equal requests of %d" % (n_req, batch)
            assert_rows(run_expand(fr, ctx, wk, fr.REQ_ONE_HOT, req, cand, None, batch, n_req, 3, what=what), expand(req, cand, mask, None), what)
        wk.close()
    finally:
        ctx.close()


# ---- 3. malformed offsets --------------------------------------------------------------------------------------------------------------------------

B_BAD = 200
MALFORMED = {
    "off[0] != 0": [3, 50, 120, B_BAD],
    "a decreasing pair": [0, 120, 50, B_BAD],
    "last entry below batch": [0, 50, 120, B_BAD - 7],
    "last entry above batch": [0, 50, 120, B_BAD + 7],
    "a negative entry": [0, -5, 120, B_BAD],
    "an entry of 2^31 - 1": [0, 50, 2 ** 31 - 1, B_BAD],
}


def check_malformed(fr, device):
    """One case per class: FR_ERR_INDEX_RANGE at sync, canaries intact, every output word one of the (distinct) input tags, and the next call on the
    worker succeeds and is exact.  In both row widths: the narrow rows share a workgroup's tile, Model-A's alternate sides word by word."""
    for kind, shared in (("narrow", np.array([0, 1, 1], np.int32)), ("A", None)):
        m, ctx = context(fr, device, kind)
        try:
            C = m.idx_cols
            shared = masks(C)["alternating"] if shared is None else shared
            ctx.set_request_columns(shared)
            mask = word_mask(shared)
            rs, rc, W = ctx.request_words(fr.REQ_ONE_HOT)
            wk = fr.Worker(ctx, 256)
            n_req = 3
            req = (np.arange(n_req * rs, dtype=np.uint32) + np.uint32(0x10000000)).reshape(n_req, rs)     # every input word a distinct tag
            cand = (np.arange(B_BAD * rc, dtype=np.uint32) + np.uint32(0x20000000)).reshape(B_BAD, rc)
            tags = np.concatenate([req.ravel(), cand.ravel()])
            good = np.array([0, 50, 120, B_BAD], np.int32)
            for what, off in MALFORMED.items():
                got = run_expand(fr, ctx, wk, fr.REQ_ONE_HOT, req, cand, off, B_BAD, n_req, W, expect=fr.FR_ERR_INDEX_RANGE, what=what)
                assert np.isin(got, tags).all(), "%s (%s): a written word is no copy of an input word" % (what, kind)
                after = "clean call after " + what
                assert_rows(run_expand(fr, ctx, wk, fr.REQ_ONE_HOT, req, cand, good, B_BAD, n_req, W, what=after), expand(req, cand, mask, good), after)
            wk.close()
        finally:
            ctx.close()


# ---- 4. equality through the existing paths -----------------------------------------------------------------------------------------------------

def valid_rows(rng, m, B, hots=None, empty_share=0.2):
    """full index rows uint32 [B][C] (hots: pooled rows [B][P], a fifth of the slots empty) inside every column's range"""
    ranges = np.asarray(m.index_ranges(), np.float64)
    if hots is not None:
        ranges = np.repeat(ranges, hots)
    rows = (rng.random((B, ranges.size)) * ranges[None, :]).astype(np.int32)
    if hots is not None:
        rows[rng.random(rows.shape) < empty_share] = -1
    return rows.view(np.uint32)


class Inputs:
    """A request-form batch whose expansion is a batch of valid lookups: request-consistent full rows, split by the context's masks."""

    def __init__(self, fr, rng, m, shared, dense_shared, B, n_req, hots=None, off=None):
        self.B, self.n_req = B, n_req
        self.off = random_offsets(rng, B, n_req) if off is None else np.asarray(off, np.int32)
        own = owners(self.off, B, n_req)
        self.mask = word_mask(shared)
        one = valid_rows(rng, m, B)
        self.req, self.cand = split(one, self.mask, self.off)
        self.full = expand(self.req, self.cand, self.mask, self.off)
        self.dense = self.req_dense = None
        if m.dense_len:
            self.dense = rng.standard_normal((B, m.dense_len)).astype(np.float32)
            if dense_shared:
                self.req_dense = rng.standard_normal((n_req, m.dense_len)).astype(np.float32)
                self.dense = self.req_dense[own]
        if hots is not None:
            self.pmask = word_mask(shared, hots)
            self.preq, self.pcand = split(valid_rows(rng, m, B, hots), self.pmask, self.off)
            self.pfull = expand(self.preq, self.pcand, self.pmask, self.off)
            w = rng.standard_normal(self.pfull.shape).astype(np.float32)
            self.wreq, self.wcand = split(w.view(np.uint32), self.pmask, self.off)
            self.wfull = expand(self.wreq, self.wcand, self.pmask, self.off)


def check_equality(fr, device, kind, precision=None):
    """Expanded rows into gather_only, submit_device, gather_pooled (unweighted, and weighted with expanded weights) and submit_pooled_device equal
    the same calls on numpy-expanded rows, bit for bit."""
    rng = np.random.default_rng(6400 + sum(map(ord, kind)))
    m, ctx = context(fr, device, kind, precision)
    bufs = []
    try:
        C, B, n_req = m.idx_cols, 301, 9
        shared = masks(C)["alternating"]
        dense_shared = bool(m.dense_len)
        hots = np.array([1, 2, 4, 3], np.int32)[np.arange(C) % 4]
        ctx.set_pooling(hots)
        ctx.set_request_columns(shared, dense_shared)
        x = Inputs(fr, rng, m, shared, dense_shared, B, n_req, hots)
        wk = fr.Worker(ctx, 512)
        dev = lambda a: bufs.append(fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a))) or bufs[-1]
        new = lambda words: bufs.append(fr.DeviceBuffer(ctx, words * 4)) or bufs[-1]
        d_off = dev(x.off)
        P = int(hots.sum())
        d_rows, d_prows, d_w = new(B * C), new(B * P), new(B * P)
        d_dense = h_dense = None
        if m.dense_len:
            h_dense = dev(x.dense)
            d_dense = new(B * m.dense_len)
            wk.expand_requests_device(B, n_req, dev(x.req_dense), None, d_dense, fr.REQ_DENSE, d_off)
        wk.expand_requests_device(B, n_req, dev(x.req), dev(x.cand), d_rows, fr.REQ_ONE_HOT, d_off)
        wk.expand_requests_device(B, n_req, dev(x.preq), dev(x.pcand), d_prows, fr.REQ_POOLED, d_off)
        wk.expand_requests_device(B, n_req, dev(x.wreq), dev(x.wcand), d_w, fr.REQ_POOLED, d_off)
        h_rows, h_prows, h_w = dev(x.full), dev(x.pfull), dev(x.wfull)
        K = m.record_len
        calls = [("gather_only", K, lambda i, d, o, w: wk.gather_only(B, i[0], d, o)),
                 ("submit_device", 1, lambda i, d, o, w: wk.submit_device(B, i[0], d, o)),
                 ("gather_pooled", K, lambda i, d, o, w: wk.gather_pooled(B, i[1], d, o)),
                 ("gather_pooled weighted", K, lambda i, d, o, w: wk.gather_pooled(B, i[1], d, o, weights=w)),
                 ("submit_pooled_device", 1, lambda i, d, o, w: wk.submit_pooled_device(B, i[1], d, o)),
                 ("submit_pooled_device weighted", 1, lambda i, d, o, w: wk.submit_pooled_device(B, i[1], d, o, weights=w))]
        for what, width, call in calls:
            res = []
            for rows, dense, wts in (((d_rows, d_prows), d_dense, d_w), ((h_rows, h_prows), h_dense, h_w)):
                d_o = fr.DeviceBuffer.from_numpy(ctx, np.zeros(B * width, np.uint32))
                call(rows, dense, d_o, wts)
                wk.sync()                       # (the first sync also completes the expansions: same worker, same stream)
                res.append(d_o.download(np.uint32, B * width))
                d_o.free()
            assert np.array_equal(res[0], res[1]), "%s (%s): %d of %d words differ" % (what, kind, int((res[0] != res[1]).sum()), res[0].size)
            assert len(set(res[1].tolist())) > B // 4, what + ": the results do not differ between items"
        wk.close()
    finally:
        for b in bufs:
            b.free()
        ctx.close()


# ---- 5. stream order -------------------------------------------------------------------------------------------------------------------------------

def check_stream_order(fr, device, group):
    """Eight batches, each expand_requests_device into its own buffer followed by push_device, one sync at the end: scores equal the same pushes
    fed host-expanded rows.  Group 64 leaves the pushes queued for a fused launch behind all eight expansions, group 1 rides the stage pipeline.
    Then the same with push_pooled_device."""
    rng = np.random.default_rng(6500 + group)
    m, ctx = context(fr, device, "A")
    bufs = []
    try:
        ctx.set_stream_group(group)
        C, B, NB, n_req = m.idx_cols, 256, 8, 5
        shared = masks(C)["first"]
        shared[C // 3] = 1
        hots = np.full(C, 2, np.int32)
        ctx.set_pooling(hots)
        ctx.set_request_columns(shared)
        wk = fr.Worker(ctx, B)
        dev = lambda a: bufs.append(fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a))) or bufs[-1]
        xs = [Inputs(fr, rng, m, shared, False, B, n_req, hots) for _ in range(NB)]
        d_sc = dev(np.zeros(NB * B, np.uint32))
        part = lambda i: d_sc.ptr.value + i * B * 4
        for what, form, W, push in (("push_device", fr.REQ_ONE_HOT, C, wk.push_device), ("push_pooled_device", fr.REQ_POOLED, 2 * C, wk.push_pooled_device)):
            pooled = form == fr.REQ_POOLED
            d_full = [dev(x.pfull if pooled else x.full) for x in xs]
            d_req = [dev(x.preq if pooled else x.req) for x in xs]
            d_cand = [dev(x.pcand if pooled else x.cand) for x in xs]
            d_off = [dev(x.off) for x in xs]
            d_out = [dev(np.zeros(B * W, np.uint32)) for _ in xs]
            d_sc.upload(np.zeros(NB * B, np.uint32))
            for i in range(NB):                  # the same pushes fed host-expanded rows
                push(B, d_full[i], None, part(i))
            wk.sync()
            want = d_sc.download(np.uint32, NB * B)
            assert len(set(want.tolist())) > B, what + ": the scores do not differ"
            d_sc.upload(np.zeros(NB * B, np.uint32))
            for i in range(NB):                  # the sequence under test: no sync before the end
                wk.expand_requests_device(B, n_req, d_req[i], d_cand[i], d_out[i], form, d_off[i])
                push(B, d_out[i], None, part(i))
            wk.sync()
            got = d_sc.download(np.uint32, NB * B)
            assert np.array_equal(got, want), "group %d, %s: %d of %d scores differ" % (group, what, int((got != want).sum()), want.size)
            for i in range(NB):
                assert np.array_equal(d_out[i].download(np.uint32, B * W).reshape(B, W), xs[i].pfull if pooled else xs[i].full)
        wk.close()
    finally:
        for b in bufs:
            b.free()
        ctx.close()


# ---- 6. the host form ------------------------------------------------------------------------------------------------------------------------------

def host_form_results(fr, device):
    """submit_requests in its three modes (and on the dense-sharing Model-C clone) + sync against infer / infer_pooled on the expanded rows; with
    fr_worker_topk between submit and sync against rank_topk.reference per request -> [(what, scores bits, (positions, score bits), expanded rows)]"""
    rng = np.random.default_rng(6600)
    out = []
    K = 6
    for kind in ("A", "C"):
        m, ctx = context(fr, device, kind)
        try:
            C, B, n_req = m.idx_cols, 200, 7
            shared = masks(C)["alternating"]
            dense_shared = bool(m.dense_len)
            hots = np.array([2, 1, 3], np.int32)[np.arange(C) % 3]
            ctx.set_pooling(hots)
            ctx.set_request_columns(shared, dense_shared)
            off = np.array([0, 0, 40, 41, 41, 120, 199, 200], np.int32)
            x = Inputs(fr, rng, m, shared, dense_shared, B, n_req, hots, off=off)
            wts, wreq, wcand = x.wfull.view(np.float32), x.wreq, x.wcand
            wk = fr.Worker(ctx, 256)
            dn = dict(req_dense=x.req_dense) if dense_shared else dict(dense=x.dense)
            runs = [("one-hot", dict(pooled=0), x.req, x.cand, lambda: wk.infer(x.full.view(np.int32), x.dense)),
                    ("pooled", dict(), x.preq, x.pcand, lambda: wk.infer_pooled(x.pfull.view(np.int32), x.dense)),
                    ("pooled weighted", dict(req_weights=wreq.view(np.float32), weights=wcand.view(np.float32)), x.preq, x.pcand,
                     lambda: wk.infer_pooled(x.pfull.view(np.int32), x.dense, weights=wts))]
            for what, kw, req, cand, plain_fn in runs:
                what = "%s, %s" % (kind, what)
                kw = dict(kw, **dn)
                plain = plain_fn().view(np.uint32)
                got = wk.infer_requests(req.view(np.int32), cand.view(np.int32), off, **kw).view(np.uint32)
                assert np.array_equal(got, plain), "%s: %d of %d scores differ from the call on expanded rows" % (what, int((got != plain).sum()), B)
                assert len(set(plain.tolist())) > B // 2, what + ": the scores do not differ"
                gi, gs = wk.infer_requests_topk(req.view(np.int32), cand.view(np.int32), off, K, **kw)
                R.assert_same((gi, gs.view(np.uint32)), R.reference(plain, K, off), "ranking after submit_requests, " + what)
                out.append((what, plain, (gi, gs.view(np.uint32))))
            wk.close()
        finally:
            ctx.close()
    return out


def expanded_rows(fr, device):
    """the expanded rows of a fixed set of inputs, to be compared across back-ends"""
    rng = np.random.default_rng(6700)
    m, ctx = context(fr, device, "A")
    try:
        C = m.idx_cols
        hots = mixed_hots(C)
        ctx.set_pooling(hots)
        shared = masks(C)["alternating"]
        ctx.set_request_columns(shared)
        wk = fr.Worker(ctx, 1024)
        res = []
        for form in (fr.REQ_ONE_HOT, fr.REQ_POOLED):
            rs, rc, W = ctx.request_words(form)
            off = random_offsets(rng, 1000, 33)
            req, cand = random_words(rng, (33, rs)), random_words(rng, (1000, rc))
            res.append(run_expand(fr, ctx, wk, form, req, cand, off, 1000, 33, W, shift=1))
        wk.close()
        return res
    finally:
        ctx.close()


# ---- 7. errors and state -----------------------------------------------------------------------------------------------------------------------------

def check_errors(fr, device):
    L = fr.lib()
    rng = np.random.default_rng(6800)
    INV, ST, OK = fr.FR_ERR_INVALID, fr.FR_ERR_STATE, fr.FR_OK
    pi = lambda a: np.ascontiguousarray(a, np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    m, ctx = context(fr, device, "C")
    try:
        C, h = m.idx_cols, ctx._h
        one = np.zeros(C, np.int32)
        one[0] = 1
        words = lambda form: L.fr_ctx_request_words(h, form, None, None, None)
        assert words(fr.REQ_ONE_HOT) == ST                                            # no split set
        old = fr.Worker(ctx, 64)                                                        # a worker older than the split
        idx = valid_rows(rng, m, 64).view(np.int32)
        dense = rng.standard_normal((64, m.dense_len)).astype(np.float32)
        before = old.infer(idx, dense).view(np.uint32)
        # fr_ctx_set_request_columns
        assert L.fr_ctx_set_request_columns(None, pi(one), C, 0) == INV
        assert L.fr_ctx_set_request_columns(h, pi(one), C - 1, 0) == INV             # a wrong n_cols
        assert L.fr_ctx_set_request_columns(h, pi(one * 2), C, 0) == INV             # a mask value other than 0/1
        assert L.fr_ctx_set_request_columns(h, pi(-one), C, 0) == INV
        assert L.fr_ctx_set_request_columns(h, pi(one), C, 2) == INV                 # dense_shared other than 0/1
        assert L.fr_ctx_set_request_columns(h, pi(one * 0), C, 0) == INV             # nothing shared at all
        assert L.fr_ctx_set_request_columns(h, pi(one * 0 + 1), C, 1) == INV         # nothing left per item
        assert L.fr_ctx_set_request_columns(h, pi(one * 0 + 1), C, 0) == OK          # (every column shared, the dense features per item)
        assert L.fr_ctx_set_request_columns(h, pi(one * 0), C, 1) == OK              # (only the dense features shared)
        d_idx = fr.DeviceBuffer.from_numpy(ctx, idx)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, dense)
        d_rec = fr.DeviceBuffer(ctx, 64 * m.record_len * 4)
        old.gather_only(64, d_idx, d_dense, d_rec)
        assert L.fr_ctx_set_request_columns(h, pi(one), C, 0) == ST                  # a worker of the context has work in flight
        assert "in flight" in L.fr_last_error().decode()
        old.sync()
        ctx.set_request_columns(one, dense_shared=True)
        assert ctx.request_words(fr.REQ_ONE_HOT) == (1, C - 1, C) and ctx.request_words(fr.REQ_DENSE) == (m.dense_len, 0, m.dense_len)
        assert words(fr.REQ_POOLED) == ST and words(3) == INV and words(-1) == INV     # the pooled form without pooling; unknown forms
        ctx.set_request_columns(one, dense_shared=False)
        assert words(fr.REQ_DENSE) == ST                                              # the dense form without dense_shared
        # the split survives set_pooling / set_pooling_modes; pooled widths follow the current hots
        hots = np.full(C, 2, np.int32)
        hots[0] = 5
        ctx.set_pooling(hots)
        assert ctx.request_words(fr.REQ_POOLED) == (5, 2 * (C - 1), 2 * C + 3) and ctx.request_words(fr.REQ_ONE_HOT) == (1, C - 1, C)
        ctx.set_pooling_modes(np.full(C, fr.POOL_MEAN, np.int32))
        assert ctx.request_words(fr.REQ_POOLED) == (5, 2 * (C - 1), 2 * C + 3)
        hots[0] = 1
        ctx.set_pooling(hots)
        assert ctx.request_words(fr.REQ_POOLED) == (1, 2 * (C - 1), 2 * C - 1)
        ctx.set_pooling(None)
        assert words(fr.REQ_POOLED) == ST and ctx.request_words(fr.REQ_ONE_HOT) == (1, C - 1, C)
        ctx.set_pooling(hots)
        # an older worker: no request buffers, the host form refuses; every existing entry point is unaffected by the split
        assert old.request_buffers() == (None, None, None, None)
        assert L.fr_worker_submit_requests(old._h, 64, 4, 0) == ST and "after fr_ctx_set_request_columns" in L.fr_last_error().decode()
        assert np.array_equal(old.infer(idx, dense).view(np.uint32), before), "infer changed with a split set"
        old.close()
        # fr_worker_expand_requests_device
        ctx.set_request_columns(one, dense_shared=True)
        wk = fr.Worker(ctx, 64)
        rs, rc, W = ctx.request_words(fr.REQ_ONE_HOT)
        d_req, d_cand = fr.DeviceBuffer.from_numpy(ctx, random_words(rng, (4, rs))), fr.DeviceBuffer.from_numpy(ctx, random_words(rng, (64, rc)))
        d_off = fr.DeviceBuffer.from_numpy(ctx, np.array([0, 16, 32, 48, 64], np.int32))
        d_reqd = fr.DeviceBuffer.from_numpy(ctx, random_words(rng, (4, m.dense_len)))
        n_out = 64 * 2 * max(C, m.dense_len)
        d_out = fr.DeviceBuffer.from_numpy(ctx, np.full(n_out, CANARY, np.uint32))

        def ex(w=wk._h, batch=64, n_req=4, off=d_off.ptr, req=d_req.ptr, cand=d_cand.ptr, form=fr.REQ_ONE_HOT, out=d_out.ptr):
            return L.fr_worker_expand_requests_device(w, batch, n_req, off, req, cand, form, out)

        for bad in (dict(w=None), dict(batch=0), dict(batch=65), dict(batch=-1), dict(n_req=0), dict(n_req=2 ** 24 + 1), dict(form=3), dict(form=-1), dict(req=None),
                    dict(out=None), dict(cand=None), dict(off=None, n_req=5)):
            assert ex(**bad) == INV, bad
        assert ex(form=fr.REQ_DENSE, req=d_reqd.ptr, cand=None) == OK                                  # (the dense form has no candidate words)
        wk.sync()
        ctx.set_pooling(None)
        assert ex(form=fr.REQ_POOLED) == ST
        ctx.set_request_columns(one, dense_shared=False)
        assert ex(form=fr.REQ_DENSE) == ST
        ctx.set_request_columns(None)                                                   # cleared
        assert ex() == ST and words(fr.REQ_ONE_HOT) == ST
        wk.sync()
        assert (d_out.download(np.uint32, n_out)[64 * m.dense_len:] == CANARY).all(), "a refused call wrote its output"
        named = wk.last_kernel()
        ctx.set_request_columns(one, dense_shared=False)
        assert ex() == OK
        wk.sync()
        assert wk.last_kernel() == named                                                # it keeps naming the last batch's kernel
        wk.close()
        # fr_worker_submit_requests: a worker created after the split but BEFORE fr_ctx_set_pooling serves the one-hot form only
        wk = fr.Worker(ctx, 64)
        ctx.set_pooling(hots)
        wk.request_buffers()[3][:5] = [0, 16, 32, 48, 64]
        for pooled in (1, 2):
            assert L.fr_worker_submit_requests(wk._h, 64, 4, pooled) == ST and "after fr_ctx_set_pooling" in L.fr_last_error().decode(), pooled
        wk.sync()                                                                       # (nothing was enqueued)
        wk.close()
        ctx.set_pooling_modes(np.full(C, fr.POOL_MEAN, np.int32))
        wk = fr.Worker(ctx, 64)
        b_idx, b_w, b_dense, b_off = wk.request_buffers()
        assert b_idx is not None and b_w is not None and b_dense is None and b_off.size == 65
        b_off[:5] = [0, 16, 32, 48, 64]
        sub = lambda batch=64, n_req=4, pooled=0: L.fr_worker_submit_requests(wk._h, batch, n_req, pooled)
        assert L.fr_worker_submit_requests(None, 64, 4, 0) == INV
        for bad in (dict(batch=0), dict(batch=65), dict(n_req=0), dict(n_req=65), dict(pooled=3), dict(pooled=-1), dict(n_req=3), dict(batch=63)):
            assert sub(**bad) == INV, bad                                               # (n_req = 3: off[3] = 48 is not the batch; batch 63: off[4] = 64 is not)
        b_off[0] = 1
        assert sub() == INV                                                             # off[0] != 0
        b_off[0] = 0
        assert sub(pooled=2) == ST and "FR_POOL_MEAN" in L.fr_last_error().decode()     # pooled weighted on a context with a MEAN column
        wk.sync()                                                                       # nothing was enqueued by any of them
        np.ctypeslib.as_array(L.fr_worker_idx_ptr(wk._h), shape=(64 * (C - 1),))[:] = idx[:, 1:].ravel()
        b_idx[:4] = idx[[0, 16, 32, 48], 0]
        wk.dense[:64] = dense
        assert sub() == OK
        assert sub() == ST                                                              # one batch in flight per worker
        wk.sync()
        wk.close()
        d = [d_idx, d_dense, d_rec, d_req, d_reqd, d_cand, d_off, d_out]
        for b in d:
            b.free()
    finally:
        ctx.close()
    c0 = fr.Context(model(fr, "C"), device=device, shard_rank=0, n_shards=2)           # a sharded context
    try:
        one = np.zeros(c0.model.idx_cols, np.int32)
        one[0] = 1
        assert L.fr_ctx_set_request_columns(c0._h, pi(one), one.size, 0) == ST
    finally:
        c0.close()
    m, ctx = context(fr, device, "narrow")                                              # an array reaching the 4000 MiB bound of the pooled calls
    try:
        ctx.set_pooling(np.array([64, 64, 1], np.int32))
        ctx.set_request_columns(np.array([1, 1, 0], np.int32))
        assert ctx.request_words(fr.REQ_POOLED) == (128, 1, 129)
        wk = fr.Worker(ctx, 16)
        d = fr.DeviceBuffer.from_numpy(ctx, np.zeros(16 * 129, np.uint32))
        big = 2 ** 24                                                                   # 2^24 request rows of 128 words: 8 GiB
        assert L.fr_worker_expand_requests_device(wk._h, 16, big, d.ptr, d.ptr, d.ptr, fr.REQ_POOLED, d.ptr) == INV and "4000 MiB" in L.fr_last_error().decode()
        wk.sync()
        d.free()
        wk.close()
    finally:
        ctx.close()
    m, ctx = context(fr, device, "A")                                                   # a model without dense features
    try:
        one = np.zeros(m.idx_cols, np.int32)
        one[0] = 1
        assert L.fr_ctx_set_request_columns(ctx._h, pi(one), one.size, 1) == INV
        assert L.fr_ctx_set_request_columns(ctx._h, pi(one * 0 + 1), one.size, 0) == INV   # nothing left per item
    finally:
        ctx.close()


# ---- 8. the server ---------------------------------------------------------------------------------------------------------------------------------

def check_server(fr, device, free_port_block):
    """fleetrec_server --requests 4 --shared-cols 20 --reply with batch 64: a block on the wire is the request rows followed by the candidate rows;
    the reply is the library's own scores of the expanded block -- or, with --topk 4, the 4 x 4 (position, score) pairs of rank_topk.reference on
    them; once with --hots 2.  Then every refused combination: exit status != 0 and the option named."""
    server = os.path.join(HOST, "fleetrec_server")
    if not os.path.exists(server):
        subprocess.check_call(["make", "-s", "-C", HOST])
    B, cap, K, S, N = 64, 200, 4, 4, 20
    m = fr.Model.builtin(fr.MODEL_A).clone(max_rows=cap)
    C = m.idx_cols
    rng = np.random.default_rng(6900)
    shared = (np.arange(C) < N).astype(np.int32)
    off = np.arange(S + 1, dtype=np.int32) * (B // S)
    blocks, plain = {}, {}
    ctx = fr.Context(m, device=device)
    try:
        ctx.fill_tables(fr.FILL_HASH, 0xF1EE7)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 99)
        for hots in (0, 2):
            if hots:
                ctx.set_pooling(np.full(C, hots, np.int32))
            wk = fr.Worker(ctx, B)
            mask = word_mask(shared, np.full(C, hots) if hots else None)
            fulls = [valid_rows(rng, m, B, np.full(C, hots) if hots else None) for _ in range(2)]
            blocks[hots] = [split(f, mask, off) for f in fulls]
            fulls = [expand(r, c, mask, off) for r, c in blocks[hots]]
            plain[hots] = [(wk.infer_pooled(f.view(np.int32)) if hots else wk.infer(f.view(np.int32))).view(np.uint32) for f in fulls]
            wk.close()
    finally:
        ctx.close()
    common = ["--model", "A", "--batch", str(B), "--threads", "1", "--tables", "hash", "--weights", "uniform", "--row-cap", str(cap), "--device", str(device)]
    form = ["--requests", str(S), "--shared-cols", str(N)]
    pair = np.dtype([("pos", "<i4"), ("score", "<u4")])
    for hots, topk in ((0, 0), (0, K), (2, 0)):
        port = free_port_block(1)
        extra = (["--topk", str(topk)] if topk else []) + (["--hots", str(hots)] if hots else [])
        srv = subprocess.Popen([server] + common + form + ["--port", str(port), "--total", "2", "--reply"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
        try:
            sk = R._connect(port, time.time() + 120)
            for (req, cand), sc in zip(blocks[hots], plain[hots]):
                sk.sendall(req.tobytes() + cand.tobytes())
                if topk:
                    got = np.frombuffer(R._recv_exact(sk, S * K * 8), pair).reshape(S, K)
                    want = R.reference(sc, K, off)
                    assert np.array_equal(got["pos"], want[0]) and np.array_equal(got["score"], want[1]), "--topk reply"
                else:
                    got = np.frombuffer(R._recv_exact(sk, B * 4), "<u4")
                    assert np.array_equal(got, sc), "hots %d: %d of %d scores differ from the library's on the expanded block" % (hots, int((got != sc).sum()), B)
            sk.close()
            out, _ = srv.communicate(timeout=120)
            assert srv.returncode == 0 and b"request-form blocks" in out and b"bytes per block" in out, out.decode()
        finally:
            if srv.poll() is None:
                srv.kill()
    refused = ((form + ["--stream"], "--stream"), (form + ["--shards", "2"], "--shards"), (form + ["--hots", "2", "--csr"], "--csr"),
               (form + ["--hots", "2", "--pool", "weighted"], "--pool weighted"), (["--requests", str(S), "--shared-cols", "0"], "--shared-cols"),
               (["--requests", str(S), "--shared-cols", str(C)], "--shared-cols"), (["--requests", "5", "--shared-cols", str(N)], "--requests"),
               (form + ["--topk", "4", "--segments", "2"], "--segments"))
    for extra, word in refused:
        r = subprocess.run([server] + common + ["--port", str(port), "--total", "1", "--reply"] + extra, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
        assert r.returncode != 0 and b"--requests" in r.stdout and word.encode() in r.stdout, (extra, r.stdout.decode())


# ---- 9. the companion code object -------------------------------------------------------------------------------------------------------------------

def check_companion(fr):
    """libfleetrec_request.so (companion.check_companion)"""
    import companion
    companion.check_companion(fr, REQUEST_LIB, ["fr_request_launch"], {"request_expand_kernel": 1}, "request_", (fr.LIB_PATH,))

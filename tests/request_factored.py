"""Factored request-form batches (fr_worker_submit_requests_factored / fr_worker_push_requests_factored_device): the checks both back-ends run
(helpers only; the tests are tests/test_cpu_request_factored.py and tests/test_gpu_request_factored.py).

The model is an exact_chain.spec record of 512 floats = 128 record words (13 tables of 8, 4, 16, 2, 32, 1, ... words and one dense word) under
FC1 512 -> 160: five 32-output tiles (two candidate workgroups per item tile, the second with one live wave), and a K at which the fp32 stage
pipeline would cut FC1's K in two (pick_nsplit: 64 groups of 8 k), so R1 entering stage 2 whole is part of what is checked.  Both splits leave 35
words on the request side and 93 on the candidate side: odd, so neither is a multiple of the kernels' k step (2 words in fp32, 4 in bf16) and the
bf16 chain pads both sides.  On exact_chain's integer data every fp32 sum is exact in any order and any split: no tolerance."""
import numpy as np

import exact_chain as E
import exact_epilogue as X

CPU = -1
SPEC = E.spec(512, (160, 64, 32), dense_len=4, name="reqfc_512")
SPLITS = {"dense shared": ((0, 3, 6, 8), True), "dense per item": ((0, 3, 5, 6, 8), False)}   # shared tables (34 + the dense word / 35 words)
SHAPES = {   # batch, offsets, split
    "1x1": (1, (0, 1), "dense shared"),
    "33x3 empty request": (33, (0, 1, 1, 33), "dense per item"),     # an owner change inside an MFMA item tile; pad items 33 .. 63
    "97x40 uneven": (97, None, "dense shared"),                      # two request tiles in the user kernel, several owners per candidate tile
    "64x4 equal": (64, (0, 16, 32, 48, 64), "dense per item"),       # the device form passes NULL offsets: the equal-requests arm of the owner rule
}
ACTS = (X.ACT_RELU, X.ACT_NONE, X.ACT_NONE)


def uneven_offsets(batch, n_req, seed=97):
    cuts = np.sort(np.random.default_rng(seed).integers(0, batch + 1, n_req - 1))
    return np.concatenate([[0], cuts, [batch]]).astype(np.int32)


class Case:
    """A context with the split set, the data loaded and one request-consistent batch: full rows + their two halves + the exact scores."""

    def __init__(self, fr, device, prec, epi, shape, max_batch=128):
        B, off, split = SHAPES[shape]
        self.B, self.off = B, uneven_offsets(B, 40) if off is None else np.asarray(off, np.int32)
        self.n_req = self.off.size - 1
        tables, dense_shared = SPLITS[split]
        self.m = m = fr.Model.from_spec(SPEC)
        data = E.make_data(SPEC, 4242)
        shared = np.zeros(m.n_tables, np.int32)
        shared[list(tables)] = 1
        sh = shared.astype(bool)
        own = np.repeat(np.arange(self.n_req), np.diff(self.off))
        self.req, full = data["idx"][100:100 + self.n_req][:, sh], data["idx"][:B].copy()
        full[:, sh] = self.req[own]
        self.cand = np.ascontiguousarray(full[:, ~sh])
        self.req_dense, self.dense = (data["dense"][100:100 + self.n_req], None) if dense_shared else (None, data["dense"][:B])
        rec = E.records(m, data, full, self.req_dense[own] if dense_shared else self.dense)
        self.ctx = ctx = fr.Context(m, device=device)
        E.load(ctx, data)
        if device != CPU:
            ctx.set_fc_precision(fr.FC_BF16 if prec == "bf16" else fr.FC_FP32)
        bs = [None] * 4
        if epi:
            bs[0] = X.make_biases(E.records(m, data, data["idx"], data["dense"]), data["ws"], 77, ACTS)[0]
            ctx.set_epilogue(0, bs[0], "relu")
            X.premise_epi(prec, rec, data["ws"], bs, ACTS + (X.ACT_NONE,))
            self.want = X.expected_epi(prec, rec, data["ws"], bs, ACTS + (X.ACT_NONE,))
        else:
            E.premise(prec, rec, data["ws"])
            self.want = E.expected(prec, rec, data["ws"])
        ctx.set_request_columns(shared, dense_shared)
        self.wk = fr.Worker(ctx, max_batch)

    def args(self):
        return self.req, self.cand, self.off

    def dense_args(self):
        return dict(req_dense=self.req_dense, dense=self.dense)

    def push(self, fr, off, n_req=None):
        """the device form on fresh device copies (off None: NULL offsets, equal requests) -> scores (sync included)"""
        bufs = []
        dev = lambda a: None if a is None else (bufs.append(fr.DeviceBuffer.from_numpy(self.ctx, np.ascontiguousarray(a))) or bufs[-1])
        d_sc = dev(np.full(self.B, np.nan, np.float32))
        try:
            self.wk.push_requests_factored_device(self.B, n_req or self.n_req, dev(self.req), dev(self.cand), d_sc, dev(off),
                                                  dev(self.req_dense), dev(self.dense))
            self.wk.sync()
            return d_sc.download(np.float32, self.B)
        finally:
            for b in bufs:
                b.free()

    def close(self):
        self.wk.close()
        self.ctx.close()


def check_shape(fr, device, prec, epi, shape):
    """(a) the exact scores of the expanded rows, (b) fr_worker_submit_requests on the same worker, the device form, and the ranking."""
    c = Case(fr, device, prec, epi, shape)
    try:
        got = c.wk.infer_requests_factored(*c.args(), **c.dense_args())
        assert np.array_equal(got, c.want), "%d of %d scores differ from the exact chain" % (int((got != c.want).sum()), c.B)
        assert np.array_equal(got, c.wk.infer_requests(*c.args(), pooled=0, **c.dense_args())), "the full-row path differs"
        assert np.array_equal(c.push(fr, None if shape.endswith("equal") else c.off), got), "the device form differs from the host form"
        if device != CPU:
            assert c.wk.last_kernel().startswith("reqfc_cand_kernel<"), c.wk.last_kernel()
        k = 3
        fi, fs = c.wk.infer_requests_factored_topk(*c.args(), k, **c.dense_args())
        ri, rs = c.wk.infer_requests_topk(*c.args(), k, pooled=0, **c.dense_args())
        assert np.array_equal(fi, ri) and np.array_equal(fs.view(np.uint32), rs.view(np.uint32))
    finally:
        c.close()


def check_malformed(fr, device):
    """A decreasing pair, then off[n_req] != batch, in the device form: FR_ERR_INDEX_RANGE at sync, and the next well-formed batch is exact.
    NULL offsets with batch % n_req != 0 are refused on the host."""
    c = Case(fr, device, "f32", False, "33x3 empty request")
    try:
        for bad in ((0, 20, 10, 33), (0, 1, 1, 32), None):
            try:
                c.push(fr, None, 2) if bad is None else c.push(fr, np.asarray(bad, np.int32))
                raise AssertionError("offsets %s were accepted" % (bad,))
            except fr.FleetRecError as e:
                assert e.status == (fr.FR_ERR_INVALID if bad is None else fr.FR_ERR_INDEX_RANGE), e
            assert np.array_equal(c.push(fr, c.off), c.want)
    finally:
        c.close()


REFUSALS = ("no split", "pooled", "fp8", "sharded")
REFUSAL_SPEC = E.spec(128, (64, 64, 64), name="reqfc_refusals")   # (widths an fp8 chain takes)


def check_refusal(fr, device, which):
    m = fr.Model.from_spec(REFUSAL_SPEC)
    shared = np.zeros(m.n_tables, np.int32)
    shared[0] = 1
    ctx = fr.Context(m, device=device, shard_rank=0, n_shards=2) if which == "sharded" else fr.Context(m, device=device)
    try:
        if which != "sharded":
            E.load(ctx, E.make_data(REFUSAL_SPEC, 4242))
        if which == "pooled":
            ctx.set_pooling(np.full(m.n_tables, 2, np.int32))
        if which == "fp8":
            ctx.set_fc_precision(fr.FC_FP8)
        if which not in ("no split", "sharded"):
            ctx.set_request_columns(shared, False)
        wk = fr.Worker(ctx, 32)
        for call in (lambda: wk.submit_requests_factored(4, 2), lambda: wk.push_requests_factored_device(4, 2, 1 << 20, 1 << 20, 1 << 20, None, None, 1 << 20)):
            try:
                call()
                raise AssertionError("%s: accepted" % which)
            except fr.FleetRecError as e:
                assert e.status == fr.FR_ERR_STATE, e
        wk.close()
    finally:
        ctx.close()

"""Shared by tests/test_cpu_pooled_refusals.py and tests/test_gpu_pooled_refusals.py: what every pooled C-ABI entry point REFUSES -- the status it
returns and the exact fr_last_error() text -- one fault at a time and for the pairs of faults whose order of checking matters.  The other pooled
suites assert the status of most of these; none pins the text or the order, which is what a change to the shared checks can alter silently.

One tiny model (shrunk Model-A, FR_INDEX_PER_TABLE, tables capped at 2000 rows), batch 16, every column's cap 2.  The set-ups, per back-end:
  none     an unsharded context without pooling (a request split set)
  main     an unsharded context: split set, a worker created BEFORE the pooling (old), then the pooling, then the worker the cases use
  mean     `main` with its last column's mode FR_POOL_MEAN for the duration of the case
  sh_none  a G = 2 pair of sharded contexts created without pooling, on the host exchange (device = -1: the CPU back-end's; GPU: the staged one)
  sh_main / sh_mean  the same pair created with pooling, all SUM / last column MEAN
Every case calls the entry point with its fault(s), keeps (status, text), then makes a clean call on the same worker and wants FR_OK from it and
from fr_worker_sync.  Refusals launch nothing: the GPU driver runs in about a second.

The expectations are tests/golden/pooled_refusals.json, a `cpu` and a `gpu` section, recorded by this module's --record switch from the case
table below against a build of the commit BEFORE the shared checks were consolidated (FR_LIB names that build); the sections say which.

The table is ENTRIES x FAULTS.  A pair that is left out is in NOT_APPLICABLE with the reason; check_table_is_whole holds the two together."""
import ctypes
import json
import os
import sys

import numpy as np

CPU = -1
B, CAP, N_REQ = 16, 2, 4
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooled_refusals.json")

DEV_PAD = ("fr_worker_gather_pooled", "fr_worker_gather_pooled_weighted", "fr_worker_submit_pooled_device", "fr_worker_submit_pooled_weighted_device",
           "fr_worker_push_pooled_device", "fr_worker_push_pooled_device_list", "fr_worker_gather_slices_pooled")
DEV_CSR = ("fr_worker_gather_pooled_csr", "fr_worker_submit_pooled_csr_device", "fr_worker_push_pooled_csr_device", "fr_worker_gather_slices_pooled_csr")
HOST = ("fr_worker_submit_pooled", "fr_worker_submit_pooled_weighted", "fr_worker_submit_pooled_csr")
REQ = ("fr_worker_submit_requests[pooled=1]", "fr_worker_submit_requests[pooled=2]")
SHARDED = ("fr_worker_submit_sharded_pooled", "fr_worker_submit_sharded_pooled_csr")
ENTRIES = DEV_PAD + DEV_CSR + HOST + REQ + SHARDED
N_ENTRY_POINTS = len({e.split("[")[0] for e in ENTRIES})      # fr_worker_submit_requests counts once: 17 C-ABI names, 18 rows
MUST_HAVE_WEIGHTS = ("fr_worker_gather_pooled_weighted", "fr_worker_submit_pooled_weighted_device")
TAKES_WEIGHTS = MUST_HAVE_WEIGHTS + DEV_CSR + ("fr_worker_push_pooled_device", "fr_worker_push_pooled_device_list", "fr_worker_gather_slices_pooled",
                                               "fr_worker_submit_pooled_weighted", "fr_worker_submit_pooled_csr", REQ[1]) + SHARDED
SLICES = ("fr_worker_gather_slices_pooled", "fr_worker_gather_slices_pooled_csr")
SUBMIT_DEV = ("fr_worker_submit_pooled_device", "fr_worker_submit_pooled_weighted_device", "fr_worker_submit_pooled_csr_device")
HOST_CSR = ("fr_worker_submit_pooled_csr", "fr_worker_submit_sharded_pooled_csr")
GATHERS = ("fr_worker_gather_pooled", "fr_worker_gather_pooled_weighted", "fr_worker_gather_pooled_csr") + SLICES

# fault -> (the entry points it applies to, the back-ends it can be provoked on)
BOTH = ("cpu", "gpu")
FAULTS = {
    "no_pooling": (ENTRIES, BOTH),
    "worker_before_pooling": (HOST + REQ, BOTH),
    "null_idx": (DEV_PAD, BOTH),
    "null_offsets": (DEV_CSR, BOTH),
    "null_out": (DEV_PAD + DEV_CSR, BOTH),
    "null_weights": (MUST_HAVE_WEIGHTS, BOTH),
    "weights_with_mean": (TAKES_WEIGHTS, BOTH),
    "nnz_negative": (DEV_CSR, BOTH),
    "nnz_null_idx": (DEV_CSR, BOTH),
    "nnz_4000mib": (DEV_CSR, BOTH),
    "bad_transport": (SLICES, BOTH),
    "lp_transport_on_cpu": (SLICES, ("cpu",)),
    "host_offsets0": (HOST_CSR + REQ, BOTH),
    "host_nnz_high": (HOST_CSR, BOTH),
    "host_nnz_negative": (HOST_CSR, BOTH),
    "pipeline_busy": (SUBMIT_DEV, ("gpu",)),
    "in_flight": (HOST + REQ + SHARDED, BOTH),
    "sharded_ctx": (tuple(e for e in DEV_PAD + DEV_CSR + HOST + REQ if e not in GATHERS), BOTH),
    "no_pooling_on_shard": (DEV_PAD + DEV_CSR + HOST, BOTH),     # a sharded context created without pooling, on an unsharded entry point
    # pairs: which of the two is reported
    "no_pooling+null_out": (DEV_PAD + DEV_CSR, BOTH),
    "null_weights+mean": (MUST_HAVE_WEIGHTS, BOTH),
    "nnz_negative+null_idx": (DEV_CSR, BOTH),
    "in_flight+host_offsets0": (HOST_CSR + REQ, BOTH),
}

# why the rest of ENTRIES x FAULTS is not in the table (fault -> [(entry points, reason)]; every pair outside FAULTS must be named here)
NOT_APPLICABLE = {
    "worker_before_pooling": [(DEV_PAD + DEV_CSR, "the device forms read none of the worker's pooled buffers: the call is legal on an older worker"),
                              (SHARDED, "a sharded context's pooling is fixed at creation: no worker predates it")],
    "null_idx": [(DEV_CSR, "the offsets form's NULL indices are the fault nnz_null_idx"), (HOST + REQ + SHARDED, "the host forms take no pointer")],
    "null_offsets": [(DEV_PAD, "the padded form has no offsets"), (HOST + REQ + SHARDED, "the host forms take no pointer")],
    "null_out": [(HOST + REQ + SHARDED, "the host forms write the worker's pinned scores")],
    "null_weights": [(tuple(e for e in ENTRIES if e not in MUST_HAVE_WEIGHTS), "only the two device *_weighted entry points make the weights mandatory: elsewhere NULL selects the unweighted fold, "
                      "and the weighted host forms read the worker's own buffer")],
    "weights_with_mean": [(tuple(e for e in ENTRIES if e not in TAKES_WEIGHTS), "the entry point has no weights")],
    "nnz_negative": [(tuple(e for e in ENTRIES if e not in DEV_CSR), "only the device offsets forms take nnz; the host forms read it from the offsets (host_nnz_*)")],
    "nnz_null_idx": [(tuple(e for e in ENTRIES if e not in DEV_CSR), "as nnz_negative")],
    "nnz_4000mib": [(tuple(e for e in ENTRIES if e not in DEV_CSR), "as nnz_negative; a host form's nnz is bounded by batch x P first")],
    "bad_transport": [(tuple(e for e in ENTRIES if e not in SLICES), "only the slice gathers take a transport")],
    "lp_transport_on_cpu": [(tuple(e for e in ENTRIES if e not in SLICES), "only the slice gathers take a transport")],
    "host_offsets0": [(tuple(e for e in ENTRIES if e not in HOST_CSR + REQ), "the entry point reads no pinned offsets (device offsets are checked by the kernel, per bag)")],
    "host_nnz_high": [(tuple(e for e in ENTRIES if e not in HOST_CSR), "the entry point reads no pinned bag offsets")],
    "host_nnz_negative": [(tuple(e for e in ENTRIES if e not in HOST_CSR), "the entry point reads no pinned bag offsets")],
    "pipeline_busy": [(GATHERS + ("fr_worker_push_pooled_device", "fr_worker_push_pooled_csr_device", "fr_worker_push_pooled_device_list"), "gathers and pushes queue behind a push: legal"),
                      (HOST + REQ + SHARDED, "a pushed batch also sets the worker in flight, which these check first: the fault in_flight")],
    "in_flight": [(DEV_PAD + DEV_CSR, "the device forms queue behind the batch in flight: legal")],
    "sharded_ctx": [(GATHERS, "a pooled gather on a shard writes the shard's slice: legal"), (SHARDED, "these are the sharded entry points")],
    "no_pooling_on_shard": [(REQ, "the missing request split is refused first, as in sharded_ctx"), (SHARDED, "their no_pooling case")],
    "no_pooling+null_out": [(HOST + REQ + SHARDED, "as null_out")],
    "null_weights+mean": [(tuple(e for e in ENTRIES if e not in MUST_HAVE_WEIGHTS), "as null_weights")],
    "nnz_negative+null_idx": [(tuple(e for e in ENTRIES if e not in DEV_CSR), "as nnz_negative")],
    "in_flight+host_offsets0": [(tuple(e for e in ENTRIES if e not in HOST_CSR + REQ), "as host_offsets0")],
}
BACKEND_ONLY = {"lp_transport_on_cpu": "a bf16 slice is legal on the GPU", "pipeline_busy": "the CPU back-end computes a push before it returns: nothing is ever queued"}


def check_table_is_whole():
    """every (entry point, fault) pair is either a case or named, with its reason, in NOT_APPLICABLE -- never both, never neither"""
    for fault, (entries, backends) in FAULTS.items():
        named = [e for es, why in NOT_APPLICABLE.get(fault, []) for e in es if why]
        assert sorted(named + list(entries)) == sorted(ENTRIES), (fault, sorted(set(ENTRIES) - set(named) - set(entries)), sorted(set(named) & set(entries)))
        assert backends == BOTH or fault in BACKEND_ONLY, fault


def cases(backend):
    return [(e, f) for f, (entries, backends) in FAULTS.items() if backend in backends for e in entries]


def _ptr(x):
    return x.ptr if hasattr(x, "ptr") else x


class Plain:
    """An unsharded context with its workers and the device copies of one good batch (both forms)."""

    def __init__(self, fr, device, pooling, X):
        self.fr, self.X = fr, X
        self.ctx = ctx = fr.Context(X.m, device=device)
        ctx.fill_tables(fr.FILL_HASH, 1)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        ctx.set_request_columns(X.shared)
        self.old = fr.Worker(ctx, B)
        if pooling:
            ctx.set_pooling(X.caps)
        self.wk = fr.Worker(ctx, B) if pooling else self.old
        self.dev = X.device_arrays(ctx, X.m.record_len)

    def set_mean(self, on):
        self.ctx.set_pooling_modes(self.X.one_mean if on else None)

    def close(self):
        for w in {self.old, self.wk}:
            w.close()
        self.ctx.close()


class Pair:
    """G = 2 sharded contexts of one device, a worker and a communicator each; the cases call rank 0."""

    def __init__(self, fr, device, hots, modes, X):
        self.fr, self.X = fr, X
        self.ctxs = [fr.Context(X.m, device=device, shard_rank=r, n_shards=2, hots=hots, modes=modes) for r in range(2)]
        for c in self.ctxs:
            c.fill_tables(fr.FILL_HASH, 1)
            c.fill_weights(fr.WEIGHTS_UNIFORM, 2)
        self.wks = [fr.Worker(c, B) for c in self.ctxs]
        self.comms = fr.Comm.init_all(self.ctxs)
        self.ctx, self.wk, self.old = self.ctxs[0], self.wks[0], self.wks[0]
        self.dev = X.device_arrays(self.ctx, max(X.m.record_len, self.ctx.shard_info()["slice_padded"]))

    def step(self, load, submit):
        """a clean step on both ranks; -> the two fr_worker_sync statuses"""
        L = self.fr.lib()
        for w in self.wks:
            load(w)
        rcs = [submit(self.wks[r]._h, self.comms[r]._h) for r in range(2)]
        return rcs + [L.fr_worker_sync(self.wks[r]._h) for r in (1, 0)]

    def close(self):
        for w in self.wks:
            w.close()
        for cm in self.comms:
            cm.close()
        for c in self.ctxs:
            c.close()


class Setups:
    def __init__(self, fr, device):
        import pooled_helpers as P
        self.fr, self.device = fr, device
        self.m = m = P.make_model(fr, 0, index_mode=0, max_rows=2000)     # 0: FR_INDEX_PER_TABLE
        C = m.idx_cols
        rng = np.random.default_rng(7300)
        self.caps = np.full(C, CAP, np.int32)
        self.one_mean = np.zeros(C, np.int32)
        self.one_mean[C - 1] = fr.POOL_MEAN
        self.shared = np.zeros(C, np.int32)
        self.shared[0] = 1
        self.rect = P.random_bags(rng, m.index_ranges(), self.caps, B, empty_share=0.3)
        self.onehot = (rng.random((B, C)) * m.index_ranges()[None, :]).astype(np.int32)
        self.dense = P.dense_for(rng, m, B)
        self.w = rng.uniform(0.5, 1.5, self.rect.shape).astype(np.float32)
        self.off, self.ind, self.wf = fr.bags_to_csr(self.rect, self.caps, weights=self.w)
        self.seg = np.arange(N_REQ + 1, dtype=np.int32) * (B // N_REQ)
        self.made = {}

    def device_arrays(self, ctx, out_floats):
        fr = self.fr
        put = lambda a: fr.DeviceBuffer.from_numpy(ctx, a)
        return dict(idx=put(self.rect), w=put(self.w), onehot=put(self.onehot), dense=put(self.dense) if self.dense is not None else None, off=put(self.off), ind=put(self.ind),
                    wf=put(self.wf), rec=fr.DeviceBuffer(ctx, B * out_floats * 4), sc=fr.DeviceBuffer(ctx, B * 4))

    def get(self, name):
        if name not in self.made:
            fr = self.fr
            if name in ("none", "main"):
                self.made[name] = Plain(fr, self.device, name == "main", self)
            else:
                self.made[name] = Pair(fr, self.device, None if name == "sh_none" else self.caps, self.one_mean if name == "sh_mean" else None, self)
        return self.made[name]

    def close(self):
        for s in self.made.values():
            s.close()
        self.made = {}


def _call(fr, S, entry, over, worker=None):
    """the entry point on set-up S with the good batch's arguments, `over` replacing some: idx / w / dense / out / off / ind / nnz / transport / weighted"""
    L, d = fr.lib(), S.dev
    h = (worker or S.wk)._h
    weighted_entry = entry in MUST_HAVE_WEIGHTS + ("fr_worker_submit_pooled_weighted", REQ[1])
    a = dict(idx=d["idx"], w=d["w"] if weighted_entry else None, dense=d["dense"], out=d["rec"] if entry in GATHERS else d["sc"], off=d["off"], ind=d["ind"], nnz=int(S.X.ind.size),
             transport=fr.FC_FP32, weighted=0)
    a.update(over)
    a = {k: _ptr(v) for k, v in a.items()}
    if entry == "fr_worker_gather_pooled":
        return L.fr_worker_gather_pooled(h, B, a["idx"], a["dense"], a["out"])
    if entry == "fr_worker_gather_pooled_weighted":
        return L.fr_worker_gather_pooled_weighted(h, B, a["idx"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_gather_pooled_csr":
        return L.fr_worker_gather_pooled_csr(h, B, a["off"], a["ind"], a["nnz"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_submit_pooled_device":
        return L.fr_worker_submit_pooled_device(h, B, a["idx"], a["dense"], a["out"])
    if entry == "fr_worker_submit_pooled_weighted_device":
        return L.fr_worker_submit_pooled_weighted_device(h, B, a["idx"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_submit_pooled_csr_device":
        return L.fr_worker_submit_pooled_csr_device(h, B, a["off"], a["ind"], a["nnz"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_push_pooled_device":
        return L.fr_worker_push_pooled_device(h, B, a["idx"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_push_pooled_csr_device":
        return L.fr_worker_push_pooled_csr_device(h, B, a["off"], a["ind"], a["nnz"], a["w"], a["dense"], a["out"])
    if entry == "fr_worker_push_pooled_device_list":
        one = lambda p: (ctypes.c_void_p * 1)(p)
        return L.fr_worker_push_pooled_device_list(h, 1, (ctypes.c_int * 1)(B), one(a["idx"]), one(a["w"]), one(a["dense"]), one(a["out"]))
    if entry == "fr_worker_gather_slices_pooled":
        return L.fr_worker_gather_slices_pooled(h, B, a["idx"], a["w"], a["dense"], a["out"], a["transport"])
    if entry == "fr_worker_gather_slices_pooled_csr":
        return L.fr_worker_gather_slices_pooled_csr(h, B, a["off"], a["ind"], a["nnz"], a["w"], a["dense"], a["out"], a["transport"])
    if entry == "fr_worker_submit_pooled":
        return L.fr_worker_submit_pooled(h, B)
    if entry == "fr_worker_submit_pooled_weighted":
        return L.fr_worker_submit_pooled_weighted(h, B)
    if entry == "fr_worker_submit_pooled_csr":
        return L.fr_worker_submit_pooled_csr(h, B, a["weighted"])
    if entry in REQ:
        return L.fr_worker_submit_requests(h, B, N_REQ, 1 + REQ.index(entry))
    if entry == "fr_worker_submit_sharded_pooled":
        return L.fr_worker_submit_sharded_pooled(h, S.comms[0]._h, B, a["weighted"])
    if entry == "fr_worker_submit_sharded_pooled_csr":
        return L.fr_worker_submit_sharded_pooled_csr(h, S.comms[0]._h, B, a["weighted"])
    raise AssertionError(entry)


def _load(S, entry, wk, weighted=False):
    """the good batch into wk's pinned buffers, in the form the host entry point reads"""
    X = S.X
    if entry in HOST_CSR:
        wk.load_pooled_csr(X.off, X.ind, X.dense, X.wf if weighted else None)
    elif entry in REQ:
        P0 = CAP   # the shared column's slots lead every pooled row
        wt = entry == REQ[1]
        wk._load_requests(X.rect[::B // N_REQ, :P0], X.rect[:, P0:], X.seg, None, X.dense, X.w[::B // N_REQ, :P0] if wt else None, X.w[:, P0:] if wt else None, 2 if wt else 1)
    elif entry in HOST + SHARDED:
        wk.load_pooled(X.rect, X.dense, X.w if (weighted or entry == "fr_worker_submit_pooled_weighted") else None)


def _clean(fr, S, entry, name, fault):
    """a clean call right after the refusal, and fr_worker_sync: -> the list of statuses (all must be FR_OK)"""
    L = fr.lib()
    own = name in ("main", "sh_main") and fault != "worker_before_pooling" and fault != "sharded_ctx"
    if isinstance(S, Pair) and (entry in SHARDED):
        if name == "sh_none":
            def load(w):
                w.idx[:B] = S.X.onehot
                if w.dense is not None:
                    w.dense[:B] = S.X.dense
            return S.step(load, lambda h, c: L.fr_worker_submit_sharded(h, c, B))
        fn = getattr(L, entry)
        return S.step(lambda w: _load(S, entry, w), lambda h, c: fn(h, c, B, 0))
    wk = S.old if fault == "worker_before_pooling" else S.wk
    if name in ("none", "sh_none"):   # (on a shard: its slice)
        rc = L.fr_worker_gather_only(wk._h, B, _ptr(S.dev["onehot"]), _ptr(S.dev["dense"]), _ptr(S.dev["rec"]))
    elif own:
        _load(S, entry, wk)
        rc = _call(fr, S, entry, {})
    else:   # a worker older than the pooling, the MEAN column, a shard: the plain pooled gather is what every one of them accepts
        rc = _call(fr, S, "fr_worker_gather_pooled", {}, worker=wk)
    return [rc, L.fr_worker_sync(wk._h)]


def run_case(fr, X, entry, fault):
    """-> (status, text) of the refused call; asserts the clean call and the sync behind it"""
    L = fr.lib()
    sharded = entry in SHARDED
    parts = fault.split("+")
    name = ("sh_" if sharded or fault in ("sharded_ctx", "no_pooling_on_shard") else "") + ("none" if "no_pooling" in parts or fault == "no_pooling_on_shard" else "mean" if sharded and ("weights_with_mean" in parts or "mean" in parts) else "main")
    S = X.get(name)
    mean = not sharded and ("weights_with_mean" in parts or "mean" in parts)
    wk = S.old if fault == "worker_before_pooling" else S.wk
    over = {}
    pinned_off = None
    if mean:
        S.set_mean(True)
    try:
        if name not in ("none", "sh_none") and fault != "worker_before_pooling" and fault != "sharded_ctx":
            _load(S, entry, wk, weighted="weights_with_mean" in parts)
        for p in parts:
            if p == "null_idx":
                over["idx"] = None
            elif p == "null_offsets":
                over["off"] = None
            elif p == "null_out":
                over["out"] = None
            elif p == "null_weights":
                over["w"] = None
            elif p == "weights_with_mean":
                over["w"], over["weighted"] = (S.dev["wf"] if entry in DEV_CSR else S.dev["w"]), 1
            elif p == "nnz_negative":
                over["nnz"] = -1
            elif p in ("nnz_null_idx", "null_idx") and entry in DEV_CSR:
                over["ind"] = None
            elif p == "nnz_4000mib":
                over["nnz"] = 1000 << 20
            elif p == "bad_transport":
                over["transport"] = 7
            elif p == "lp_transport_on_cpu":
                over["transport"] = fr.FC_BF16
            elif p in ("host_offsets0", "host_nnz_high", "host_nnz_negative"):
                pinned_off = wk.request_buffers()[3] if entry in REQ else wk.pool_offsets
                C = X.m.idx_cols
                pos, val = {"host_offsets0": (0, 1), "host_nnz_high": (B * C, B * C * CAP + 1), "host_nnz_negative": (B * C, -1)}[p]
                pinned_off[pos] = val
            elif p == "pipeline_busy":
                assert _call(fr, S, "fr_worker_push_pooled_device", {}) == fr.FR_OK
            elif p == "in_flight":
                assert _call(fr, S, "fr_worker_gather_pooled", {}) == fr.FR_OK
        if "nnz_negative+null_idx" == fault:
            over["ind"] = None
        rc = _call(fr, S, entry, over, worker=wk)
        text = L.fr_last_error().decode()
        if "pipeline_busy" in parts or "in_flight" in parts:
            assert L.fr_worker_sync(wk._h) == fr.FR_OK, L.fr_last_error().decode()
        assert rc != fr.FR_OK, "%s accepted %s" % (entry, fault)
        if mean:
            S.set_mean(False)
            mean = False
        after = _clean(fr, S, entry, name, fault)
        assert after == [fr.FR_OK] * len(after), (entry, fault, after, L.fr_last_error().decode())
        return rc, text
    finally:
        if mean:
            S.set_mean(False)


def golden(backend):
    with open(GOLDEN) as f:
        return json.load(f)[backend]["cases"]


def run_all(fr, device):
    """-> {"entry|fault": [status, text]} for every case of the back-end"""
    check_table_is_whole()
    backend = "cpu" if device == CPU else "gpu"
    X = Setups(fr, device)
    got = {}
    try:
        for entry, fault in cases(backend):
            got["%s|%s" % (entry, fault)] = list(run_case(fr, X, entry, fault))
    finally:
        X.close()
    return got


def check_refusals(fr, device):
    backend = "cpu" if device == CPU else "gpu"
    want = golden(backend)
    got = run_all(fr, device)
    covered = {k.split("|")[0].split("[")[0] for k in got}
    print("pooled refusals (%s): %d cases over %d C-ABI entry points" % (backend, len(got), len(covered)))
    assert len(covered) == N_ENTRY_POINTS == 17, sorted(covered)
    assert sorted(got) == sorted(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    wrong = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not wrong, wrong


if __name__ == "__main__":
    # python tests/pooled_refusals.py --record cpu|gpu COMMIT "MACHINE" [OUT.json]: run with FR_LIB naming a build of COMMIT; rewrites that section of the golden file
    if len(sys.argv) < 5 or sys.argv[1] != "--record" or sys.argv[2] not in BOTH:
        sys.exit("usage: FR_LIB=<build of COMMIT> python tests/pooled_refusals.py --record cpu|gpu COMMIT MACHINE [OUT.json]")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import __graft_entry__ as g
    out = sys.argv[5] if len(sys.argv) > 5 else GOLDEN
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc[sys.argv[2]] = {"recorded_from": sys.argv[3], "machine": sys.argv[4], "library": "FR_LIB" if os.environ.get("FR_LIB") else "the tree's own build",
                        "cases": run_all(g.load_package(), CPU if sys.argv[2] == "cpu" else 0)}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d %s cases into %s" % (len(doc[sys.argv[2]]["cases"]), sys.argv[2], out))

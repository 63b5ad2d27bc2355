"""Shared by tests/test_cpu_key_refusals.py and tests/test_gpu_key_refusals.py: what every keyed C-ABI entry point (key spaces, the list-form changes
of a map, its life cycle, row pools, the resolves) and the two fr_*_update_rows forms REFUSE -- the status and the exact fr_last_error() text -- one
fault at a time and for the pairs of faults whose order of checking matters; and, in a second table, what fr_worker_sync and the host forms SAY about
the bits of a status word (fr_index_range_fail).  The other keyed suites assert the status of most of these and a substring of some texts; none pins the
text or the order, which is what a change to the shared checks can alter silently.

One tiny model (key_admit.model: tables of 50 / 1500 / 90 rows), batch 16, lists of at most 8 keys.  The set-ups, per back-end:
  main     an unsharded context: a worker created BEFORE the first key space (old), then column 0 left FR_KEYS_ROWS, column 1 MAPPED (max_keys 2) with
           a row pool of 2 rows, column 2 MAPPED (max_keys 2) without a pool, then the worker the cases use.  No split, no pooling.
  split    an unsharded context with a request split and pooling (the shared column 32 hots): the 4000 MiB bound of the resolve
  sharded  a G = 2 pair of shard contexts of one device, a worker on rank 0
  fused    (GPU only) a shrunk Model-A, which streams through the fused item-tile kernel: host-fed batches can be queued on its worker
Before every case the columns of `main` are put back as they started (keys 5 and 6 live in both maps).  Every case calls the entry point with its
fault(s), keeps (status, text), then makes a clean call on the same objects and wants FR_OK from it and from fr_worker_sync.  Refusals launch
nothing and the status cases launch a handful of one-block kernels.

The expectations are tests/golden/key_refusals.json, a `cpu` and a `gpu` section, recorded by this module's --record switch from the tables below
against a build of the commit BEFORE the keyed host code was consolidated (FR_LIB names that build); the sections say which.

The first table is ENTRIES x FAULTS.  A pair that is left out is in NOT_APPLICABLE with the reason; check_table_is_whole holds the two together."""
import ctypes
import json
import os
import sys

import numpy as np

CPU = -1
B = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "key_refusals.json")
KEYS, ROWS = (5, 6), (3, 4)          # the pairs both maps hold before every case (the pool column: admitted, rows 10 and 11)
POOL_FIRST, POOL_ROWS, MAX_KEYS = 10, 2, 2

MUT_W = ("fr_worker_put_keys", "fr_worker_erase_keys", "fr_worker_admit_keys")
MUT_C = ("fr_ctx_put_keys", "fr_ctx_erase_keys", "fr_ctx_admit_keys")
MUT = MUT_W + MUT_C
ERASE = ("fr_worker_erase_keys", "fr_ctx_erase_keys")
ADMIT = ("fr_worker_admit_keys", "fr_ctx_admit_keys")
SET_SPACE, REBUILD, SET_POOL = ("fr_ctx_set_key_space",), ("fr_ctx_rebuild_key_space",), ("fr_ctx_set_row_pool",)
CTX_SET = SET_SPACE + REBUILD + SET_POOL                   # the three calls guarded by fr_pooling_busy
GETTERS = ("fr_ctx_key_space", "fr_ctx_row_pool")
STATS, EXPORT = ("fr_ctx_key_space_stats",), ("fr_ctx_export_keys",)
RESOLVE, SUBMIT, MISSES = ("fr_worker_resolve_keys_device",), ("fr_worker_submit_keyed",), ("fr_worker_key_misses",)
UPD_W, UPD_C = ("fr_worker_update_rows",), ("fr_ctx_update_rows",)
KEYED = SET_SPACE + GETTERS[:1] + MUT + STATS + EXPORT + REBUILD + SET_POOL + GETTERS[1:] + RESOLVE + SUBMIT + MISSES
ENTRIES = KEYED + UPD_W + UPD_C
HAS_COL = CTX_SET + GETTERS + MUT + STATS + EXPORT + UPD_W + UPD_C     # (the updates: their table)
NEEDS_MAP = MUT + STATS + EXPORT + REBUILD + SET_POOL
HAS_ROWS = tuple(e for e in MUT if e not in ERASE) + EXPORT + RESOLVE + UPD_W + UPD_C
ALIGNED_ROWS = tuple(e for e in MUT if e not in ERASE) + RESOLVE + UPD_W

# the argument names of every entry point, in order (h: the worker or the context; p*: out-pointers that may be NULL)
SIG = {
    "fr_ctx_set_key_space": ("h", "col", "mode", "seed", "max_keys", "miss_row"), "fr_ctx_key_space": ("h", "col", "p1", "p2", "p3", "p4", "p5"),
    "fr_worker_put_keys": ("h", "col", "n", "keys", "rows"), "fr_ctx_put_keys": ("h", "col", "n", "keys", "rows"),
    "fr_worker_erase_keys": ("h", "col", "n", "keys"), "fr_ctx_erase_keys": ("h", "col", "n", "keys"),
    "fr_worker_admit_keys": ("h", "col", "n", "keys", "rows"), "fr_ctx_admit_keys": ("h", "col", "n", "keys", "rows"),
    "fr_ctx_key_space_stats": ("h", "col", "p1", "p2", "p3", "p4"), "fr_ctx_export_keys": ("h", "col", "cap", "keys", "rows", "n_out"),
    "fr_ctx_rebuild_key_space": ("h", "col", "seed", "max_keys"), "fr_ctx_set_row_pool": ("h", "col", "first", "n_rows"),
    "fr_ctx_row_pool": ("h", "col", "p1", "p2", "p3"), "fr_worker_resolve_keys_device": ("h", "n", "rows_kind", "pooled", "keys", "rows"),
    "fr_worker_submit_keyed": ("h", "n", "pooled"), "fr_worker_key_misses": ("h", "out", "reset"),
    "fr_worker_update_rows": ("h", "col", "n", "keys", "rows"), "fr_ctx_update_rows": ("h", "col", "n", "keys", "rows"),
}

# fault -> (the entry points it applies to, the back-ends it can be provoked on)
BOTH = ("cpu", "gpu")
FAULTS = {
    "null_handle": (ENTRIES, BOTH),
    "col_minus1": (HAS_COL, BOTH),
    "col_high": (HAS_COL, BOTH),
    "n_negative": (MUT + UPD_W + UPD_C, BOTH),
    "null_keys": (MUT + EXPORT + RESOLVE + UPD_W + UPD_C, BOTH),
    "null_rows": (HAS_ROWS, BOTH),
    "null_out": (MISSES, BOTH),
    "no_map": (NEEDS_MAP, BOTH),                       # a ROWS column
    "no_pool": (ADMIT, BOTH),                          # a MAPPED column without a pool
    "misaligned_keys": (MUT + RESOLVE, BOTH),          # + 4 bytes
    "misaligned_rows": (ALIGNED_ROWS, BOTH),           # + 2 bytes
    "host_fed_queued": (MUT_W + UPD_W, ("gpu",)),      # after fr_worker_push_host, no flush
    "in_flight": (CTX_SET + SUBMIT, BOTH),
    "sharded_ctx": (CTX_SET + MUT + STATS + EXPORT + RESOLVE + SUBMIT, BOTH),
    "bad_mode": (SET_SPACE, BOTH),
    "max_keys_0": (SET_SPACE + REBUILD, BOTH),
    "max_keys_high": (SET_SPACE + REBUILD, BOTH),      # 2^30 + 1
    "max_keys_below_live": (REBUILD, BOTH),
    "bad_miss_row": (SET_SPACE, BOTH),
    "pool_n_negative": (SET_POOL, BOTH),
    "pool_leaves_column": (SET_POOL, BOTH),
    "pool_contains_miss_row": (SET_POOL, BOTH),
    "cap_negative": (EXPORT, BOTH),
    "cap_below_live": (EXPORT, BOTH),
    "rows_kind_bad": (RESOLVE, BOTH),
    "pooled_bad": (RESOLVE + SUBMIT, BOTH),
    "n_rows_0": (RESOLVE + SUBMIT, BOTH),
    "bound_4000mib": (RESOLVE, BOTH),
    "no_split": (RESOLVE, BOTH),
    "no_pooling": (RESOLVE + SUBMIT, BOTH),
    "worker_before_key_space": (SUBMIT, BOTH),
    # pairs: which of the two is reported
    "col_high+n_negative": (MUT + UPD_W + UPD_C, BOTH),
    "n_negative+null_keys": (MUT + UPD_W + UPD_C, BOTH),
    "null_rows+no_map": (tuple(e for e in MUT if e not in ERASE), BOTH),
    "no_map+no_pool": (ADMIT, BOTH),
    "n0+misaligned_keys": (MUT + UPD_W + UPD_C, BOTH),              # -> FR_OK: an empty list passes whatever the pointers are
    "misaligned_keys+host_fed_queued": (MUT_W, ("gpu",)),
    "sharded_ctx+in_flight": (CTX_SET, BOTH),
    "max_keys_0+col_high": (SET_SPACE + REBUILD, BOTH),
}
# the cases whose call is accepted on purpose: (entry point or None for all, fault, back-end or None for both)
ACCEPTED = ((None, "n0+misaligned_keys", None),
            ("fr_worker_update_rows", "misaligned_rows", "cpu"))    # the CPU back-end computes the update before the alignment check, as ever


def _rest(*groups):
    named = {e for g in groups for e in g}
    return tuple(e for e in ENTRIES if e not in named)


# why the rest of ENTRIES x FAULTS is not in the table (fault -> [(entry points, reason)]; every pair outside FAULTS must be named here)
NOT_APPLICABLE = {
    "col_minus1": [(_rest(HAS_COL), "the entry point takes no column")],
    "col_high": [(_rest(HAS_COL), "the entry point takes no column")],
    "n_negative": [(_rest(MUT, UPD_W, UPD_C), "the entry point takes no list length (the resolve's row count is n_rows_0, the export's cap cap_negative)")],
    "null_keys": [(_rest(MUT, EXPORT, RESOLVE, UPD_W, UPD_C), "the entry point takes no key (or row id) list")],
    "null_rows": [(_rest(HAS_ROWS), "the entry point takes no rows list")],
    "null_out": [(_rest(MISSES), "every other out-pointer may be NULL (the getters, the stats, n_out) or is the fault null_rows")],
    "no_map": [(SET_SPACE + GETTERS, "legal on a ROWS column: the one makes the map, the others report the column as it is"),
               (RESOLVE + SUBMIT + MISSES, "a resolve reads ROWS columns as rows: legal"), (UPD_W + UPD_C, "a row update takes a table, not a key space")],
    "no_pool": [(_rest(ADMIT), "only an admit needs the pool; an erase without one is the plain erase")],
    "misaligned_keys": [(_rest(MUT, RESOLVE), "the entry point takes no 64-bit key list (the export writes through memcpy)")],
    "misaligned_rows": [(_rest(ALIGNED_ROWS), "the entry point takes no rows list, or reads a host list through memcpy (fr_ctx_update_rows, fr_ctx_export_keys)")],
    "host_fed_queued": [(_rest(MUT_W, UPD_W), "only the stream-ordered worker forms are ordered against the worker's queued batches "
                                              "(fr_worker_resolve_keys_device and fr_worker_submit_keyed: an in-flight worker, the fault in_flight)")],
    "in_flight": [(_rest(CTX_SET, SUBMIT), "legal beside work in flight: the worker forms queue behind it, the host forms run on the set-up stream, the readers idle the device")],
    "sharded_ctx": [(GETTERS + MISSES, "legal on a shard: every column reports FR_KEYS_ROWS, no pool, no miss"), (UPD_W + UPD_C, "row updates are legal on a shard (resident tables)")],
    "bad_mode": [(_rest(SET_SPACE), "only fr_ctx_set_key_space takes a mode")],
    "max_keys_0": [(_rest(SET_SPACE, REBUILD), "the entry point takes no max_keys")],
    "max_keys_high": [(_rest(SET_SPACE, REBUILD), "the entry point takes no max_keys")],
    "max_keys_below_live": [(_rest(REBUILD), "only a rebuild has live keys to keep; fr_ctx_set_key_space starts empty")],
    "bad_miss_row": [(_rest(SET_SPACE), "only fr_ctx_set_key_space takes a miss_row")],
    "pool_n_negative": [(_rest(SET_POOL), "only fr_ctx_set_row_pool takes a row range")],
    "pool_leaves_column": [(_rest(SET_POOL), "only fr_ctx_set_row_pool takes a row range")],
    "pool_contains_miss_row": [(_rest(SET_POOL), "only fr_ctx_set_row_pool takes a row range")],
    "cap_negative": [(_rest(EXPORT), "only the export takes a cap")],
    "cap_below_live": [(_rest(EXPORT), "only the export takes a cap")],
    "rows_kind_bad": [(_rest(RESOLVE), "only the device resolve takes a rows_kind")],
    "pooled_bad": [(_rest(RESOLVE, SUBMIT), "the entry point takes no pooled flag")],
    "n_rows_0": [(_rest(RESOLVE, SUBMIT), "the entry point takes no row count (a list of 0 keys is legal: n0+misaligned_keys)")],
    "bound_4000mib": [(_rest(RESOLVE), "fr_worker_submit_keyed is bounded by the worker's batch first; no other entry point sizes a key matrix")],
    "no_split": [(_rest(RESOLVE), "only the device resolve takes request / candidate rows")],
    "no_pooling": [(_rest(RESOLVE, SUBMIT), "the entry point takes no pooled flag")],
    "worker_before_key_space": [(_rest(SUBMIT), "only fr_worker_submit_keyed reads the worker's pinned key buffer")],
    "col_high+n_negative": [(_rest(MUT, UPD_W, UPD_C), "as n_negative")],
    "n_negative+null_keys": [(_rest(MUT, UPD_W, UPD_C), "as n_negative")],
    "null_rows+no_map": [(_rest(MUT) + ERASE, "as null_rows and no_map")],
    "no_map+no_pool": [(_rest(ADMIT), "as no_pool")],
    "n0+misaligned_keys": [(_rest(MUT, UPD_W, UPD_C), "as n_negative")],
    "misaligned_keys+host_fed_queued": [(_rest(MUT_W), "as host_fed_queued; fr_worker_update_rows takes no 64-bit list")],
    "sharded_ctx+in_flight": [(_rest(CTX_SET), "as in_flight; fr_worker_submit_keyed's own worker cannot be in flight on another context")],
    "max_keys_0+col_high": [(_rest(SET_SPACE, REBUILD), "as max_keys_0")],
}
BACKEND_ONLY = {"host_fed_queued": "the CPU back-end has no host-fed streaming: nothing is ever queued",
                "misaligned_keys+host_fed_queued": "as host_fed_queued"}

# ---- the second table: the texts of a status word ------------------------------------------------------------------------------------------------------
# cause -> the kind of call that raises it; through a worker the bits wait for fr_worker_sync, through the context they are the call's own answer
CAUSES = {"lookup": "lookup", "update": "update", "put_minus1": "put", "put_bad_row": "put", "put_full": "put", "erase_minus1": "erase", "admit_minus1": "admit",
          "admit_no_row": "admit", "admit_full": "admit"}
WORKER_PAIRS = ("lookup+put_minus1", "put_bad_row+erase_minus1", "admit_minus1+put_full", "admit_no_row+erase_minus1", "admit_full+lookup")
NEXT_KIND = {"update": "put", "put": "erase", "erase": "admit", "admit": "update"}      # the clean host-form call that follows a refused one: one status word


def status_cases():
    return ["worker|" + c for c in tuple(CAUSES) + WORKER_PAIRS] + ["ctx|" + c for c in CAUSES if c != "lookup"]


def check_table_is_whole():
    """every (entry point, fault) pair is either a case or named, with its reason, in NOT_APPLICABLE -- never both, never neither"""
    assert sorted(SIG) == sorted(ENTRIES) and len(KEYED) == 16 and len(set(ENTRIES)) == 18
    for fault, (entries, backends) in FAULTS.items():
        named = [e for es, why in NOT_APPLICABLE.get(fault, []) for e in es if why]
        assert sorted(named + list(entries)) == sorted(ENTRIES), (fault, sorted(set(ENTRIES) - set(named) - set(entries)), sorted(set(named) & set(entries)))
        assert backends == BOTH or fault in BACKEND_ONLY, fault
    for pair in WORKER_PAIRS:
        assert all(c in CAUSES for c in pair.split("+")), pair


def cases(backend):
    return [(e, f) for f, (entries, backends) in FAULTS.items() if backend in backends for e in entries]


def _accepted(entry, fault, backend):
    return any(e in (None, entry) and f == fault and b in (None, backend) for e, f, b in ACCEPTED)


# ---- the set-ups -------------------------------------------------------------------------------------------------------------------------------------

class Setup:
    """A context with its workers, the host lists and their device copies.  The three columns the cases name: `pool` (the widest: MAPPED with a row
    pool), `map` (the next: MAPPED without one), `rows` (the third: left FR_KEYS_ROWS).  keyed=False: no key space is ever set (a shard, the split)."""

    def __init__(self, fr, device, model, batch=B, keyed=True, shard=None, split=False, stream_group=0):
        self.fr, self.m, self.batch, self.keyed = fr, model, batch, keyed
        self.ctx = ctx = fr.Context(model, device=device, **(dict(shard_rank=shard, n_shards=2) if shard is not None else {}))
        ctx.fill_tables(fr.FILL_HASH, 7)
        ctx.fill_weights(fr.WEIGHTS_UNIFORM, 11)
        if stream_group:
            ctx.set_stream_group(stream_group)
        self.ranges = model.index_ranges()
        self.C = len(self.ranges)
        order = [int(i) for i in np.argsort(-self.ranges, kind="stable")]
        self.pool, self.map, self.rows = order[0], order[1], order[2]
        if split:
            shared, hots = np.zeros(self.C, np.int32), np.ones(self.C, np.int32)
            shared[0], hots[0] = 1, 32
            ctx.set_request_columns(shared)
            ctx.set_pooling(hots)
        self.old = fr.Worker(ctx, batch)
        if keyed:
            self.restore()
        self.wk = fr.Worker(ctx, batch) if keyed else self.old
        put = lambda a: fr.DeviceBuffer.from_numpy(ctx, a)
        # host lists (the key list starts 8 bytes into its array, the rows list 4: a misaligned pointer still lies inside) and their device copies
        self.hk = np.array([0] + list(KEYS) + [0] * 7, np.int64)
        self.hr = np.array([0] + list(ROWS) + [0] * 9, np.int32)
        self.hr_out = np.full(12, -7, np.int32)
        self.dk, self.dr, self.dr_out = put(self.hk), put(self.hr), put(self.hr_out)
        self.ek, self.er = np.zeros(8, np.int64), np.zeros(8, np.int32)                      # the export's
        dim = int(model.tables()[0].dim)
        self.table_rows = int(model.rows()[0])
        self.uid = np.zeros(4, np.int32)                                                       # a row update of table 0: row 0 <- zeros
        self.urow = np.zeros(4 + dim + 4, np.float32)
        self.duid, self.durow = put(self.uid), put(self.urow)
        res = np.zeros((batch, self.C), np.int64)                                             # a resolve / a keyed batch every column accepts
        if keyed:
            res[:, self.pool], res[:, self.map] = KEYS[0], KEYS[1]
        self.res = res
        self.dres, self.didx = put(np.concatenate([np.zeros(1, np.int64), res.reshape(-1)])), put(np.zeros(1 + batch * self.C, np.int32))
        self.dgood, bad = put(np.zeros((batch, self.C), np.int32)), np.zeros((batch, self.C), np.int32)
        bad[0, self.rows] = int(self.ranges[self.rows])
        self.dbad = put(bad)
        out_floats = max(int(model.record_len), int(ctx.shard_info()["slice_padded"]) if shard is not None else 0)
        self.drec = fr.DeviceBuffer(ctx, batch * out_floats * 4)
        self.bufs = [self.dk, self.dr, self.dr_out, self.duid, self.durow, self.dres, self.didx, self.dgood, self.dbad, self.drec]
        self.scores = np.zeros(batch, np.float32)

    def restore(self):
        """the columns as every case finds them: both maps hold KEYS (the pool column's admitted), the third column is FR_KEYS_ROWS"""
        fr, ctx = self.fr, self.ctx
        ctx.set_key_space(self.rows, fr.KEYS_ROWS)
        ctx.set_key_space(self.pool, fr.KEYS_MAPPED, 1, MAX_KEYS, -1)
        ctx.set_key_space(self.map, fr.KEYS_MAPPED, 2, MAX_KEYS, -1)
        ctx.set_row_pool(self.pool, POOL_FIRST, POOL_ROWS)
        ctx.put_keys(self.map, KEYS, ROWS)
        assert sorted(ctx.admit_keys(self.pool, KEYS).tolist()) == [POOL_FIRST, POOL_FIRST + 1]

    def gather(self, idx=None):
        """one launch on the worker: it is in flight until the next sync"""
        return self.fr.lib().fr_worker_gather_only(self.wk._h, self.batch, (self.dgood if idx is None else idx).ptr.value, None, self.drec.ptr.value)

    def push_host(self):
        rng = np.random.default_rng(7400)
        self.wk.push_host((rng.random((self.batch, self.C)) * self.ranges[None, :]).astype(np.int32), None, self.scores)
        assert self.wk.host_pending()[0] == 1

    def good(self, entry):
        """the arguments of a call that entry accepts, by name"""
        fr, dev = self.fr, entry.startswith("fr_worker_")
        a = dict(h=(self.wk if dev else self.ctx)._h, col=self.map, n=len(KEYS), p1=None, p2=None, p3=None, p4=None, p5=None, reset=0)
        a["keys"], a["rows"] = (self.dk.ptr.value if dev else self.hk.ctypes.data) + 8, (self.dr.ptr.value if dev else self.hr.ctypes.data) + 4
        if entry in ADMIT:
            a["col"], a["rows"] = self.pool, (self.dr_out.ptr.value if dev else self.hr_out.ctypes.data) + 4
        elif entry in SET_SPACE:
            a.update(mode=fr.KEYS_MAPPED, seed=2, max_keys=MAX_KEYS, miss_row=-1)
        elif entry in REBUILD:
            a.update(seed=3, max_keys=MAX_KEYS)
        elif entry in SET_POOL:
            a.update(col=self.pool, first=POOL_FIRST, n_rows=POOL_ROWS)
        elif entry in GETTERS + STATS:
            a["col"] = self.pool
        elif entry in EXPORT:
            self.n_out = ctypes.c_int64(-5)
            a.update(col=self.pool, cap=8, keys=self.ek.ctypes.data, rows=self.er.ctypes.data, n_out=ctypes.byref(self.n_out))
        elif entry in RESOLVE:
            a.update(n=self.batch, rows_kind=fr.KEY_ROWS_FULL, pooled=0, keys=self.dres.ptr.value + 8, rows=self.didx.ptr.value + 4)
        elif entry in SUBMIT:
            p = fr.lib().fr_worker_key_ptr(self.wk._h)
            if p:   # (a worker older than the first key space, or of a shard, has no key buffer)
                np.ctypeslib.as_array(p, shape=(self.res.size,))[:] = self.res.reshape(-1)
            a.update(n=self.batch, pooled=0)
        elif entry in MISSES:
            self.misses = ctypes.c_uint64(0)
            a["out"] = ctypes.byref(self.misses)
        elif entry in UPD_W + UPD_C:
            a.update(col=0, n=1, keys=self.duid.ptr.value if dev else self.uid.ctypes.data, rows=(self.durow.ptr.value if dev else self.urow.ctypes.data) + 16)
        return a

    def call(self, entry, over=None, worker=None):
        a = self.good(entry)
        a.update(over or {})
        if worker is not None and a["h"] is not None:
            a["h"] = worker._h
        return getattr(self.fr.lib(), entry)(*[a[k] for k in SIG[entry]])

    def sync(self):
        return self.fr.lib().fr_worker_sync(self.wk._h)

    def close(self):
        for b in self.bufs:
            b.free()
        for w in {self.old, self.wk}:
            w.close()
        self.ctx.close()


class Setups:
    def __init__(self, fr, device):
        self.fr, self.device, self.made = fr, device, {}

    def get(self, name):
        if name not in self.made:
            import key_admit as KA
            fr = self.fr
            if name == "fused":   # (key_admit.check_arguments' model: it streams through the fused item-tile kernel)
                self.made[name] = Setup(fr, self.device, fr.Model.builtin(fr.MODEL_A).clone(row_scale=0.001, max_rows=2000), batch=256, stream_group=64)
            elif name == "sharded":
                self.other = fr.Context(KA.model(fr), device=self.device, shard_rank=1, n_shards=2)
                self.made[name] = Setup(fr, self.device, KA.model(fr), keyed=False, shard=0)
            else:
                self.made[name] = Setup(fr, self.device, KA.model(fr), keyed=name == "main", split=name == "split")
        return self.made[name]

    def close(self):
        for s in self.made.values():
            s.close()
        if "sharded" in self.made:
            self.other.close()
        self.made = {}


# ---- the first table ---------------------------------------------------------------------------------------------------------------------------------------

def run_case(fr, X, entry, fault, backend):
    """-> (status, text) of the refused call; asserts the clean call and the sync behind it"""
    L = fr.lib()
    parts = fault.split("+")
    S = X.get("sharded" if "sharded_ctx" in parts else "fused" if "host_fed_queued" in parts else "split" if fault == "bound_4000mib" else "main")
    if S.keyed:
        S.restore()
    S.hr_out[:] = -7
    over, worker = {}, None
    for p in parts:
        if p == "null_handle":
            over["h"] = None
        elif p == "col_minus1":
            over["col"] = -1
        elif p == "col_high":
            over["col"] = S.C if entry not in UPD_W + UPD_C else int(S.m.n_tables)
        elif p == "n_negative":
            over["n"] = -1
        elif p == "n0":
            over["n"] = 0
        elif p == "null_keys":
            over["keys"] = None
        elif p == "null_rows":
            over["rows"] = None
        elif p == "null_out":
            over["out"] = None
        elif p == "no_map":
            over["col"] = S.rows
        elif p == "no_pool":
            over.setdefault("col", S.map)                # (no_map+no_pool: the ROWS column has neither)
        elif p == "misaligned_keys":
            over["keys"] = S.good(entry)["keys"] + 4
        elif p == "misaligned_rows":
            over["rows"] = S.good(entry)["rows"] + 2
        elif p == "host_fed_queued":
            S.push_host()
        elif p == "in_flight":
            assert S.gather() == fr.FR_OK
        elif p == "bad_mode":
            over["mode"] = 7
        elif p == "max_keys_0":
            over["max_keys"] = 0
        elif p == "max_keys_high":
            over["max_keys"] = 2 ** 30 + 1
        elif p == "max_keys_below_live":
            over.update(col=S.pool, max_keys=1)
        elif p == "bad_miss_row":
            over["miss_row"] = int(S.ranges[S.map])
        elif p == "pool_n_negative":
            over["n_rows"] = -1
        elif p == "pool_leaves_column":
            over.update(first=int(S.ranges[S.pool]) - 1, n_rows=2)
        elif p == "pool_contains_miss_row":
            S.ctx.set_key_space(S.pool, fr.KEYS_MAPPED, 1, MAX_KEYS, POOL_FIRST + 1)
        elif p == "cap_negative":
            over["cap"] = -1
        elif p == "cap_below_live":
            over["cap"] = 1
        elif p == "rows_kind_bad":
            over["rows_kind"] = 3
        elif p == "pooled_bad":
            over["pooled"] = 3
        elif p == "n_rows_0":
            over["n"] = 0
        elif p == "bound_4000mib":
            over.update(n=1 << 24, rows_kind=fr.KEY_ROWS_REQUEST, pooled=1)
        elif p == "no_split":
            over["rows_kind"] = fr.KEY_ROWS_CANDIDATE
        elif p == "no_pooling":
            over["pooled"] = 1
        elif p == "worker_before_key_space":
            worker = S.old
    d_before = S.dr_out.download(np.int32, 12)
    rc = S.call(entry, over, worker)
    text = L.fr_last_error().decode() if rc != fr.FR_OK else ""
    if entry in EXPORT:
        text += " | n_out = %d" % S.n_out.value
    assert (rc == fr.FR_OK) == _accepted(entry, fault, backend), "%s, %s: status %d (%s)" % (entry, fault, rc, text)
    if "in_flight" in parts or "host_fed_queued" in parts:
        assert S.sync() == fr.FR_OK, L.fr_last_error().decode()
    if rc != fr.FR_OK and entry in ADMIT:
        assert (S.hr_out == -7).all() and np.array_equal(S.dr_out.download(np.int32, 12), d_before), "%s, %s: a refused admit wrote rows_out" % (entry, fault)
    if worker is not None:
        assert L.fr_worker_sync(worker._h) == fr.FR_OK
    if S.keyed:
        S.restore()
    after = [S.gather() if "sharded_ctx" in parts else S.call(entry), S.sync()]
    assert after == [fr.FR_OK] * 2, (entry, fault, after, L.fr_last_error().decode())
    return rc, text


# ---- the second table ----------------------------------------------------------------------------------------------------------------------------------------

def _raise(fr, S, cause, via):
    """one call that marks `cause` in a status word -> its status (a worker form: FR_OK, the bits wait for the sync)"""
    dev = via == "worker"
    kind = CAUSES[cause]
    if cause == "lookup":
        return S.gather(S.dbad)
    if cause == "update":
        ids = np.array([S.table_rows, 0, 0, 0], np.int32)
        S.tmp = [fr.DeviceBuffer.from_numpy(S.ctx, ids)] if dev else [ids]
        S.bufs.extend(S.tmp if dev else [])
        return S.call("fr_%s_update_rows" % via, dict(keys=S.tmp[0].ptr.value if dev else ids.ctypes.data))
    keys, rows, col = {"put_minus1": ([-1, KEYS[0]], [3, 3], S.map), "put_bad_row": ([KEYS[0]], [int(S.ranges[S.map])], S.map), "put_full": ([7], [3], S.map),
                       "erase_minus1": ([-1, KEYS[0]], None, S.map), "admit_minus1": ([-1, KEYS[0]], None, S.pool), "admit_no_row": ([7], None, S.pool),
                       "admit_full": ([7], None, S.pool)}[cause]
    if cause == "admit_full":   # a dead key holds its place in the map, its row is back in the pool: a new key finds a row and no place
        S.ctx.erase_keys(S.pool, [KEYS[1]])
    hk, hr = np.array([0] + keys + [0] * 6, np.int64), np.array([0] + (rows or [0, 0]) + [0] * 6, np.int32)
    over = dict(col=col, n=len(keys))
    if dev:
        S.tmp = [fr.DeviceBuffer.from_numpy(S.ctx, hk), fr.DeviceBuffer.from_numpy(S.ctx, hr)]
        S.bufs.extend(S.tmp)
        over["keys"] = S.tmp[0].ptr.value + 8
        if kind == "put":
            over["rows"] = S.tmp[1].ptr.value + 4
    else:
        S.tmp = [hk, hr]
        over["keys"] = hk.ctypes.data + 8
        if kind == "put":
            over["rows"] = hr.ctypes.data + 4
    return S.call("fr_%s_%s_keys" % (via, kind), over)


def _clean_host_call(fr, S, kind):
    return S.call("fr_ctx_update_rows") if kind == "update" else S.call("fr_ctx_%s_keys" % kind)


def run_status_case(fr, X, name):
    """-> (status, text): of fr_worker_sync behind the worker forms, of the call itself through the context"""
    L = fr.lib()
    S = X.get("main")
    S.restore()
    via, causes = name.split("|")
    if via == "worker":
        for cause in causes.split("+"):
            assert _raise(fr, S, cause, via) == fr.FR_OK, (name, cause, L.fr_last_error().decode())
        rc = S.sync()
        text = L.fr_last_error().decode()
        assert S.sync() == fr.FR_OK, "%s: the worker's status word was not cleared by the sync that reported it" % name
    else:
        rc = _raise(fr, S, causes, via)
        text = L.fr_last_error().decode()
        # the call reported its own bits and left none: the next clean host-form call, of another kind, shares the one status word
        after = _clean_host_call(fr, S, NEXT_KIND[CAUSES[causes]])
        assert after == fr.FR_OK and S.sync() == fr.FR_OK, (name, after, L.fr_last_error().decode())
    assert rc == fr.FR_ERR_INDEX_RANGE, (name, rc, text)
    S.restore()
    after = [_clean_host_call(fr, S, k) for k in NEXT_KIND] + [S.call(e) for e in MUT_W + UPD_W] + [S.sync()]
    assert after == [fr.FR_OK] * len(after), (name, after, L.fr_last_error().decode())
    return rc, text


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------------------

def golden(backend):
    with open(GOLDEN) as f:
        return json.load(f)[backend]


def run_all(fr, device):
    """-> ({"entry|fault": [status, text]}, {"worker|causes" / "ctx|cause": [status, text]}) for every case of the back-end"""
    check_table_is_whole()
    backend = "cpu" if device == CPU else "gpu"
    X = Setups(fr, device)
    got, status = {}, {}
    try:
        for entry, fault in cases(backend):
            got["%s|%s" % (entry, fault)] = list(run_case(fr, X, entry, fault, backend))
        for name in status_cases():
            status[name] = list(run_status_case(fr, X, name))
    finally:
        X.close()
    return got, status


def check_refusals(fr, device):
    backend = "cpu" if device == CPU else "gpu"
    want = golden(backend)
    got, status = run_all(fr, device)
    covered = {k.split("|")[0] for k in got}
    print("key refusals (%s): %d cases over %d C-ABI entry points, %d status-word cases" % (backend, len(got), len(covered), len(status)))
    assert sorted(covered) == sorted(ENTRIES)
    assert not fr.lib().fr_worker_key_ptr(None)      # the seventeenth keyed entry point returns a pointer, not a status: NULL for NULL
    for have, rec in ((got, want["cases"]), (status, want["status"])):
        assert sorted(have) == sorted(rec), (sorted(set(have) - set(rec)), sorted(set(rec) - set(have)))
        wrong = {k: (have[k], rec[k]) for k in have if have[k] != rec[k]}
        assert not wrong, wrong


if __name__ == "__main__":
    # python tests/key_refusals.py --record cpu|gpu COMMIT "MACHINE" [OUT.json]: run with FR_LIB naming a build of COMMIT; rewrites that section of the golden file
    if len(sys.argv) < 5 or sys.argv[1] != "--record" or sys.argv[2] not in BOTH:
        sys.exit("usage: FR_LIB=<build of COMMIT> python tests/key_refusals.py --record cpu|gpu COMMIT MACHINE [OUT.json]")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import __graft_entry__ as g
    out = sys.argv[5] if len(sys.argv) > 5 else GOLDEN
    doc = json.load(open(out)) if os.path.exists(out) else {}
    got, status = run_all(g.load_package(), CPU if sys.argv[2] == "cpu" else 0)
    doc[sys.argv[2]] = {"recorded_from": sys.argv[3], "machine": sys.argv[4], "library": "FR_LIB" if os.environ.get("FR_LIB") else "the tree's own build",
                        "cases": got, "status": status}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d + %d %s cases into %s" % (len(got), len(status), sys.argv[2], out))

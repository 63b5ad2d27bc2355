"""Keyed lookups (fr_ctx_set_key_space / fr_*_put_keys / fr_worker_resolve_keys_device / fr_worker_submit_keyed): the checks, stated once and
parameterised by device; the tests are tests/test_cpu_keyed.py (device = -1) and tests/test_gpu_keyed.py.  The reference is the contract in plain
Python: a dict per MAPPED column and mix64 on Python integers (Spaces.row).  A batch draws its keys from a pool of a few dozen keys per column --
every special value among them -- so the reference is computed once per (column, key) and spread over the batch with numpy.  Every comparison is
np.array_equal; nothing here has a tolerance: the resolve produces integers, and everything behind it is the code that runs on pre-resolved rows."""
import ctypes
import os

import numpy as np

import rank_topk as R
import request_form as Q

CPU = -1
ROOT = Q.ROOT
KEYS_LIB = os.path.join(ROOT, "gpu-fpga-recommendation-system_amd", "libfleetrec_keys.so")
BATCHES = Q.BATCHES        # 1, 63, 64, 65, 301, 4097: around a wave, past a workgroup's chunk of 1024 words at every width used here
GUARD = 64                 # canary words on either side of the output
CANARY = 0x5a5a5a5a
M64 = (1 << 64) - 1
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
NO_ROW = 0x7fffffff
# 0, -2, the ends of int64, the three values around the largest row number, and pairs that differ only above bit 32
SPECIAL = [0, -2, I64_MIN, I64_MAX, 2 ** 31 - 2, 2 ** 31 - 1, 2 ** 31, 5, 5 + 2 ** 32, 2 ** 33 + 7, 2 ** 34 + 7, 7 - 2 ** 40]


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------

def mix64(z):
    z &= M64
    z ^= z >> 30
    z = z * 0xbf58476d1ce4e5b9 & M64
    z ^= z >> 27
    z = z * 0x94d049bb133111eb & M64
    return z ^ (z >> 31)


def slots_of(max_keys):
    s = 2
    while s < 2 * max_keys:
        s *= 2
    return s


def home(key, seed, slots):
    return mix64((key & M64) ^ seed) & (slots - 1)


class Spaces:
    """The key spaces of a context, mirrored: set() / put() call the library AND keep the reference (a dict per MAPPED column)."""

    def __init__(self, fr, ctx, m):
        self.fr, self.ctx, self.ranges = fr, ctx, [int(r) for r in m.index_ranges()]
        self.mode = [fr.KEYS_ROWS] * len(self.ranges)
        self.seed, self.max_keys, self.miss, self.map = [0] * len(self.ranges), [0] * len(self.ranges), [NO_ROW] * len(self.ranges), [None] * len(self.ranges)

    def set(self, col, mode, seed=0, max_keys=0, miss_row=NO_ROW):
        self.ctx.set_key_space(col, mode, seed, max_keys, miss_row)
        self.mode[col], self.seed[col], self.max_keys[col], self.miss[col] = mode, seed, max_keys, miss_row
        self.map[col] = {} if mode == self.fr.KEYS_MAPPED else None

    def cycle(self, rng, max_keys=48, miss_kinds=("row", -1, NO_ROW)):
        """columns cycle through ROWS / HASHED / MAPPED (a single column is MAPPED), the MAPPED ones' miss_row through a row, -1 and FR_KEY_NO_ROW"""
        fr, n = self.fr, 0
        for c, r in enumerate(self.ranges):
            mode = (fr.KEYS_ROWS, fr.KEYS_HASHED, fr.KEYS_MAPPED)[c % 3 if len(self.ranges) > 1 else 2]
            if mode == fr.KEYS_MAPPED:
                kind = miss_kinds[n % len(miss_kinds)]
                n += 1
                self.set(c, mode, int(rng.integers(0, 2 ** 63)), max_keys, int(rng.integers(0, r)) if kind == "row" else kind)
            elif mode == fr.KEYS_HASHED:
                self.set(c, mode, int(rng.integers(0, 2 ** 63)))

    def put(self, col, keys, rows, via=None):
        """legal pairs only; via: a function (col, keys, rows) that makes the library's call (default: Context.put_keys)"""
        (via or self.ctx.put_keys)(col, keys, rows)
        for k, r in zip(keys, rows):
            self.map[col][int(k)] = int(r)

    def row(self, col, key):
        """-> (row, miss)"""
        fr, key = self.fr, int(key)
        if key == -1:
            return -1, False
        if self.mode[col] == fr.KEYS_ROWS:
            return (key if 0 <= key < 2 ** 31 - 1 else NO_ROW), False
        if self.mode[col] == fr.KEYS_HASHED:
            return ((mix64((key & M64) ^ self.seed[col]) >> 32) * self.ranges[col]) >> 32, False
        return (self.map[col][key], False) if key in self.map[col] else (self.miss[col], True)


class Pools:
    """Per column a pool of keys -- the specials, -1, keys present in the column's map (put here), absent ones, small row-like numbers -- with the
    reference's row and miss flag of each; draw() makes a batch and its reference."""

    def __init__(self, rng, sp, present=16, absent=8, valid_only=False):
        """valid_only: every key of the pool resolves to a row inside its column (for batches that go through a gather): no special, no -1, and on a
        MAPPED column whose miss_row is no row, no absent key"""
        fr = sp.fr
        self.keys, self.rows, self.miss = [], [], []
        for c, r in enumerate(sp.ranges):
            small = [int(x) for x in rng.integers(0, r, size=8)]
            far = [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=absent, dtype=np.int64) if int(x) != -1]
            pool = list(small)
            if sp.mode[c] == fr.KEYS_MAPPED:
                have = [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=present, dtype=np.int64) if int(x) != -1] + small[:4]
                have = list(dict.fromkeys(have))
                sp.put(c, have, [int(x) for x in rng.integers(0, r, size=len(have))])
                pool = have + (far if not valid_only or 0 <= sp.miss[c] < r else [])
            elif sp.mode[c] == fr.KEYS_HASHED:
                pool = small + far
            if not valid_only:
                pool = pool + SPECIAL + [-1, -1, -1]
            self.keys.append(np.array(pool, np.int64))
            ref = [sp.row(c, k) for k in pool]
            self.rows.append(np.array([x[0] for x in ref], np.int64).astype(np.int32))
            self.miss.append(np.array([x[1] for x in ref], bool))

    def draw(self, rng, n_rows, wcol):
        """wcol: the index column of every word of a row -> (keys int64 [n_rows][W], rows int32 [n_rows][W], misses)"""
        keys, rows = np.empty((n_rows, len(wcol)), np.int64), np.empty((n_rows, len(wcol)), np.int32)
        misses = 0
        for w, c in enumerate(wcol):
            pick = rng.integers(0, len(self.keys[c]), size=n_rows)
            keys[:, w], rows[:, w] = self.keys[c][pick], self.rows[c][pick]
            misses += int(self.miss[c][pick].sum())
        return keys, rows, misses


def word_cols(C, rows_kind, shared=None, hots=None):
    """the index column of every word of a row of the given kind (0 full, 1 request, 2 candidate)"""
    cols = [c for c in range(C) if rows_kind == 0 or (bool(shared[c]) == (rows_kind == 1))]
    return [c for c in cols for _ in range(int(hots[c]) if hots is not None else 1)]


# ---- one resolve, its output between canaries -----------------------------------------------------------------------------------------------------

def run_resolve(fr, ctx, wk, keys, rows_kind=0, pooled=False, expect=None, what=""):
    """One fr_worker_resolve_keys_device + sync -> int32 rows of keys' shape.  The key array starts 8 bytes past a 16-byte boundary; the 64 canary
    words on either side of the output must be untouched."""
    keys = np.ascontiguousarray(keys, np.int64)
    d_keys = fr.DeviceBuffer.from_numpy(ctx, np.concatenate([np.zeros(1, np.int64), keys.reshape(-1)]))
    d_out = fr.DeviceBuffer.from_numpy(ctx, np.full(2 * GUARD + keys.size, CANARY, np.uint32))
    try:
        assert d_keys.ptr.value % 16 == 0
        wk.resolve_keys_device(len(keys), d_keys.ptr.value + 8, d_out.ptr.value + 4 * GUARD, rows_kind, pooled)
        got = R.status_of(fr, wk.sync)
        assert got == (fr.FR_OK if expect is None else expect), "%s: sync returned %d" % (what, got)
        a = d_out.download(np.uint32, 2 * GUARD + keys.size)
        assert (a[:GUARD] == CANARY).all() and (a[GUARD + keys.size:] == CANARY).all(), "%s: a canary around the output was written" % what
        return a[GUARD:GUARD + keys.size].view(np.int32).reshape(keys.shape)
    finally:
        d_keys.free()
        d_out.free()


def assert_rows(got, want, what):
    assert got.shape == want.shape and np.array_equal(got, want), "%s: %d of %d rows differ" % (what, int((got != want).sum()), want.size)


# ---- 1. words --------------------------------------------------------------------------------------------------------------------------------------

WORD_CASES = ("A", "C", "C_bank", "C_item", "narrow")


def check_words(fr, device, kind):
    """Every rows_kind x one-hot / pooled of one index mode, every batch size, keys of every class, against the reference; the misses add up."""
    assert mix64(5) == 13168350753275463132 and mix64(4) == 13232826040865663252
    rng = np.random.default_rng(7100 + sum(map(ord, kind)))
    m, ctx = Q.context(fr, device, kind)
    try:
        C = m.idx_cols
        sp = Spaces(fr, ctx, m)
        sp.cycle(rng)
        pools = Pools(rng, sp)
        hots = Q.mixed_hots(C)
        ctx.set_pooling(hots)
        shared = np.zeros(C, np.int32) if C == 1 else Q.masks(C)["alternating"]
        if C > 1:
            ctx.set_request_columns(shared)
        wk = fr.Worker(ctx, max(BATCHES))
        want_misses = 0
        forms = [(k, p) for k in ((0, 1, 2) if C > 1 else (0,)) for p in (False, True)]
        for n, B in enumerate(BATCHES):
            for rows_kind, pooled in forms if B != 4097 else forms[:1] + forms[3:4]:   # (the largest batch: full one-hot rows and pooled request rows)
                wcol = word_cols(C, rows_kind, shared, hots if pooled else None)
                if rows_kind != 0:
                    words = ctx.request_words(fr.REQ_POOLED if pooled else fr.REQ_ONE_HOT)
                    assert len(wcol) == words[rows_kind - 1]
                keys, rows, misses = pools.draw(rng, B, wcol)
                what = "%s, rows_kind %d, pooled %d, batch %d" % (kind, rows_kind, pooled, B)
                assert_rows(run_resolve(fr, ctx, wk, keys, rows_kind, pooled, what=what), rows, what)
                want_misses += misses
        assert wk.key_misses() == want_misses and want_misses > 0
        wk.close()
    finally:
        ctx.close()


# ---- 2. probe chains -----------------------------------------------------------------------------------------------------------------------------

def check_probe_chains(fr, device):
    """Maps of max_keys 1, 2, 8, 1000 filled to exactly max_keys keys, up to five of which share the LAST slot as their home (found by search on
    the host), so the chain wraps; present and absent keys on and beside the chain resolve as the dict says."""
    rng = np.random.default_rng(7200)
    m, ctx = Q.context(fr, device, "narrow")
    try:
        sp = Spaces(fr, ctx, m)
        wk = fr.Worker(ctx, 2048)
        col, R_c = 2, sp.ranges[2]
        for max_keys in (1, 2, 8, 1000):
            seed, slots = 0x1234 + max_keys, slots_of(max_keys)
            sp.set(col, fr.KEYS_MAPPED, seed, max_keys, 3)
            on_chain = []
            k = 1
            while len(on_chain) < 9:     # keys whose home is the last slot: the first few go into the map, the rest are absent keys ON the chain
                if home(k, seed, slots) == slots - 1:
                    on_chain.append(k)
                k += 1
            n_chain = min(max_keys, 5)
            others = []
            while n_chain + len(others) < max_keys:
                x = int(rng.integers(I64_MIN, I64_MAX, dtype=np.int64))
                if x != -1 and x not in others and x not in on_chain:
                    others.append(x)
            have = on_chain[:n_chain] + others
            sp.put(col, have, [int(x) for x in rng.integers(0, R_c, size=len(have))])    # one call: the chain's keys race for the same slots
            assert ctx.key_space(col) == (fr.KEYS_MAPPED, seed, max_keys, max_keys, 3)
            absent = on_chain[n_chain:] + [int(x) for x in rng.integers(I64_MIN, I64_MAX, size=40, dtype=np.int64) if int(x) not in have and int(x) != -1]
            ask = np.array(have + absent + [-1], np.int64)
            keys = np.full((len(ask), 3), -1, np.int64)
            keys[:, col] = ask
            want = np.full(keys.shape, -1, np.int32)
            want[:, col] = [sp.row(col, x)[0] for x in ask]
            what = "max_keys %d" % max_keys
            assert_rows(run_resolve(fr, ctx, wk, keys, what=what), want, what)
            assert wk.key_misses() == len(absent), what
        wk.close()
    finally:
        ctx.close()


# ---- 3. puts ---------------------------------------------------------------------------------------------------------------------------------------

def check_puts(fr, device):
    rng = np.random.default_rng(7300)
    m, ctx = Q.context(fr, device, "narrow")
    bufs = []
    try:
        sp = Spaces(fr, ctx, m)
        col, R_c, MAXK = 1, sp.ranges[1], 16
        sp.set(col, fr.KEYS_MAPPED, 77, MAXK, -1)
        wk = fr.Worker(ctx, 256)
        dev = lambda a: bufs.append(fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a))) or bufs[-1]

        def by_worker(c, keys, rows):   # the device form + sync
            wk.put_keys(c, len(keys), dev(np.asarray(keys, np.int64)), dev(np.asarray(rows, np.int32)))
            wk.sync()

        def resolved(ask):
            keys = np.full((len(ask), 3), -1, np.int64)
            keys[:, col] = ask
            return run_resolve(fr, ctx, wk, keys)[:, col]

        def check(ask, what):
            assert np.array_equal(resolved(ask), np.array([sp.row(col, k)[0] for k in ask], np.int32)), what

        first = [11, -7, I64_MIN, I64_MAX, 2 ** 40]
        sp.put(col, first, [1, 2, 3, 4, 5], via=by_worker)                      # insert
        check(first + [12, 0], "insert")
        sp.put(col, [11, I64_MAX, -7], [60, 69, -1], via=by_worker)              # overwrite two, forget one (its row becomes miss_row)
        check(first + [12], "overwrite / forget")
        assert ctx.key_space(col)[3] == 5, "a forgotten key keeps its slot"
        sp.put(col, [-7], [9])                                                   # ... and can be given a row again (host form)
        check(first, "put after forget")
        ctx.put_keys(col, [500, 500, 500, 501], [21, 22, 23, 24])                # a key listed three times in one call
        got = resolved([500, 501])
        assert got[0] in (21, 22, 23) and got[1] == 24 and ctx.key_space(col)[3] == 7, got
        sp.map[col][500], sp.map[col][501] = int(got[0]), 24
        # an illegal row and a -1 key among good pairs: reported, every other pair applied
        for via in ("ctx", "worker"):
            base = 600 if via == "ctx" else 700
            keys, rows = [base, base + 1, -1, base + 2, base + 3, base + 4], [1, R_c, 2, -2, NO_ROW, 3]
            if via == "ctx":
                assert R.status_of(fr, lambda: ctx.put_keys(col, keys, rows)) == fr.FR_ERR_INDEX_RANGE
            else:
                wk.put_keys(col, len(keys), dev(np.array(keys, np.int64)), dev(np.array(rows, np.int32)))
                assert R.status_of(fr, wk.sync) == fr.FR_ERR_INDEX_RANGE
            msg = fr.lib().fr_last_error().decode()
            assert "key put" in msg and "FR_KEY_EMPTY" in msg and "miss_row" in msg and "max_keys" not in msg, msg
            sp.map[col][base], sp.map[col][base + 4] = 1, 3
            check([base, base + 1, base + 2, base + 3, base + 4], "good pairs beside bad ones, " + via)
            wk.sync()                                                            # the sticky word was cleared: the worker is usable
        assert ctx.key_space(col)[3] == 11
        # overflow by one and by many
        fill = [1000 + i for i in range(MAXK - 11)]
        sp.put(col, fill, [int(x) for x in rng.integers(0, R_c, size=len(fill))], via=by_worker)
        assert ctx.key_space(col)[3] == MAXK
        everything = list(sp.map[col])
        assert R.status_of(fr, lambda: ctx.put_keys(col, [2000], [1])) == fr.FR_ERR_INDEX_RANGE and "max_keys" in fr.lib().fr_last_error().decode()
        wk.put_keys(col, 40, dev(np.arange(3000, 3040, dtype=np.int64)), dev(np.ones(40, np.int32)))
        assert R.status_of(fr, wk.sync) == fr.FR_ERR_INDEX_RANGE and "max_keys" in fr.lib().fr_last_error().decode()
        assert ctx.key_space(col)[3] == MAXK
        check(everything + [2000, 3000, 3039], "after the overflowing puts")
        sp.put(col, [everything[0]], [33], via=by_worker)                        # a full map still takes a present key
        check(everything, "overwrite in a full map")
        # stream order on one worker: resolve, put, resolve, one sync
        sp.set(col, fr.KEYS_MAPPED, 78, MAXK, 5)
        sp.put(col, [1, 2, 3], [10, 20, 30])
        ask = np.array([1, 2, 3, 4, 5], np.int64)
        keys = np.full((5, 3), -1, np.int64)
        keys[:, col] = ask
        d_keys, d_a, d_b = dev(keys), dev(np.zeros(15, np.int32)), dev(np.zeros(15, np.int32))
        before = [sp.row(col, k)[0] for k in ask]
        wk.resolve_keys_device(5, d_keys, d_a)
        wk.put_keys(col, 3, dev(np.array([2, 4, 3], np.int64)), dev(np.array([21, 41, 5], np.int32)))
        wk.resolve_keys_device(5, d_keys, d_b)
        wk.sync()
        sp.map[col].update({2: 21, 4: 41, 3: 5})
        assert list(d_a.download(np.int32, 15).reshape(5, 3)[:, col]) == before == [10, 20, 30, 5, 5]
        assert list(d_b.download(np.int32, 15).reshape(5, 3)[:, col]) == [10, 21, 5, 41, 5]
        # the host form beside a worker in flight
        wk.resolve_keys_device(5, d_keys, d_a)
        sp.put(col, [5, 1], [55, 11])
        wk.sync()
        a = d_a.download(np.int32, 15).reshape(5, 3)[:, col]
        assert a[0] in (10, 11) and a[4] in (5, 55) and list(a[1:4]) == [21, 5, 41], a     # per key the old or the new row
        check([1, 2, 3, 4, 5, 6], "after fr_ctx_put_keys beside a worker in flight")
        wk.close()
    finally:
        for b in bufs:
            b.free()
        ctx.close()


# ---- 4. equality through the existing paths ------------------------------------------------------------------------------------------------------

def check_equality(fr, device, kind, precision=None, pooled=0):
    """submit_keyed gives the scores of submit / submit_pooled[_weighted] on the reference's rows, bit for bit; a FR_KEY_NO_ROW miss in a one-hot
    batch is FR_ERR_INDEX_RANGE at sync and leaves the worker usable."""
    rng = np.random.default_rng(7400 + sum(map(ord, kind)))
    m, ctx = Q.context(fr, device, kind, precision)
    try:
        C, B = m.idx_cols, 301
        sp = Spaces(fr, ctx, m)
        sp.cycle(rng, miss_kinds=("row", -1) if pooled else ("row",))
        hots = np.array([1, 2, 4, 3], np.int32)[np.arange(C) % 4] if pooled else None
        if pooled:
            ctx.set_pooling(hots)
        pools = Pools(rng, sp, valid_only=True)
        wk = fr.Worker(ctx, 512)
        keys, rows, _ = pools.draw(rng, B, word_cols(C, 0, hots=hots))
        dense = rng.standard_normal((B, m.dense_len)).astype(np.float32) if m.dense_len else None
        if pooled:
            empty = rng.random(keys.shape) < 0.2
            keys[empty], rows[empty] = -1, -1
            wts = rng.standard_normal(keys.shape).astype(np.float32) if pooled == 2 else None
            got, want = wk.infer_pooled_keyed(keys, dense, wts), wk.infer_pooled(rows, dense, weights=wts)
        else:
            got, want = wk.infer_keyed(keys, dense), wk.infer(rows, dense)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: %d of %d scores differ" % (kind, int((got != want).sum()), B)
        assert len(set(want.view(np.uint32).tolist())) > B // 4, "the scores do not differ between items"
        if not pooled:
            col = next(c for c in range(C) if sp.mode[c] == fr.KEYS_MAPPED) if C >= 3 else 0
            sp.set(col, fr.KEYS_MAPPED, 3, 64, NO_ROW)
            bad = keys.copy()
            bad[B // 2, col] = 123456789                                          # absent: resolves to FR_KEY_NO_ROW
            assert R.status_of(fr, lambda: wk.infer_keyed(bad, dense)) == fr.FR_ERR_INDEX_RANGE
            assert "outside its table" in fr.lib().fr_last_error().decode()
            sp.put(col, [int(k) for k in set(keys[:, col].tolist())], [0] * len(set(keys[:, col].tolist())))
            rows[:, col] = 0
            again, want = wk.infer_keyed(keys, dense), wk.infer(rows, dense)
            assert np.array_equal(again.view(np.uint32), want.view(np.uint32)), "the worker is not usable after the index-range error"
        wk.close()
    finally:
        ctx.close()


# ---- 5. the request form ---------------------------------------------------------------------------------------------------------------------------

def check_request_form(fr, device):
    """Resolving REQUEST and CANDIDATE rows and expanding them gives the rows of expanding the KEYS on the host and resolving FULL rows, one-hot and
    pooled; the scores behind both are equal."""
    rng = np.random.default_rng(7500)
    m, ctx = Q.context(fr, device, "A")
    bufs = []
    try:
        C, B, n_req = m.idx_cols, 301, 9
        sp = Spaces(fr, ctx, m)
        sp.cycle(rng, miss_kinds=("row", -1))
        hots = np.array([1, 2, 4, 3], np.int32)[np.arange(C) % 4]
        shared = Q.masks(C)["alternating"]
        ctx.set_pooling(hots)
        ctx.set_request_columns(shared)
        pools = Pools(rng, sp, valid_only=True)
        wk = fr.Worker(ctx, 512)
        dev = lambda a: bufs.append(fr.DeviceBuffer.from_numpy(ctx, np.ascontiguousarray(a))) or bufs[-1]
        off = Q.random_offsets(rng, B, n_req)
        own = Q.owners(off, B, n_req)
        d_off = dev(off)
        for pooled in (False, True):
            h = hots if pooled else None
            mask = Q.word_mask(shared, h)
            rk, rrows, _ = pools.draw(rng, n_req, word_cols(C, 1, shared, h))
            ck, crows, _ = pools.draw(rng, B, word_cols(C, 2, shared, h))
            W = mask.size
            full = np.empty((B, W), np.int64)
            full[:, mask], full[:, ~mask] = rk[own], ck
            want = np.empty((B, W), np.int32)
            want[:, mask], want[:, ~mask] = rrows[own], crows
            d_r, d_c, d_x, d_f = dev(np.zeros(rk.size, np.int32)), dev(np.zeros(ck.size, np.int32)), dev(np.zeros(B * W, np.int32)), dev(np.zeros(B * W, np.int32))
            d_s1, d_s2 = dev(np.zeros(B, np.uint32)), dev(np.zeros(B, np.uint32))
            submit = wk.submit_pooled_device if pooled else wk.submit_device
            wk.resolve_keys_device(n_req, dev(rk), d_r, fr.KEY_ROWS_REQUEST, pooled)     # no sync before the scores: one stream orders the four launches
            wk.resolve_keys_device(B, dev(ck), d_c, fr.KEY_ROWS_CANDIDATE, pooled)
            wk.expand_requests_device(B, n_req, d_r, d_c, d_x, fr.REQ_POOLED if pooled else fr.REQ_ONE_HOT, d_off)
            submit(B, d_x, None, d_s1)
            wk.sync()
            wk.resolve_keys_device(B, dev(full), d_f, fr.KEY_ROWS_FULL, pooled)
            submit(B, d_f, None, d_s2)
            wk.sync()
            x, f = d_x.download(np.int32, B * W).reshape(B, W), d_f.download(np.int32, B * W).reshape(B, W)
            assert_rows(x, want, "resolve, then expand (pooled %d)" % pooled)
            assert_rows(f, want, "expand on the host, then resolve (pooled %d)" % pooled)
            s1, s2 = d_s1.download(np.uint32, B), d_s2.download(np.uint32, B)
            assert np.array_equal(s1, s2) and len(set(s1.tolist())) > B // 4
        wk.close()
    finally:
        for b in bufs:
            b.free()
        ctx.close()


# ---- 6. the host form and top-K ---------------------------------------------------------------------------------------------------------------------

def host_form_results(fr, device):
    """-> [(what, resolved rows, scores bits, (positions, score bits))] of fixed keyed batches through submit_keyed (+ fr_worker_topk), checked here
    against the plain host forms on the reference's rows and against rank_topk.reference; compared across back-ends by the GPU test."""
    out = []
    K = 6
    off = np.array([0, 0, 40, 41, 41, 120, 199, 200], np.int32)
    for kind, pooled in (("A", 0), ("C", 0), ("A", 2)):
        rng = np.random.default_rng(7600 + pooled)
        m, ctx = Q.context(fr, device, kind)
        try:
            C, B = m.idx_cols, 200
            sp = Spaces(fr, ctx, m)
            sp.cycle(rng, miss_kinds=("row", -1) if pooled else ("row",))
            hots = np.array([2, 1, 3], np.int32)[np.arange(C) % 3] if pooled else None
            if pooled:
                ctx.set_pooling(hots)
            pools = Pools(rng, sp, valid_only=True)
            wk = fr.Worker(ctx, 256)
            keys, rows, _ = pools.draw(rng, B, word_cols(C, 0, hots=hots))
            dense = rng.standard_normal((B, m.dense_len)).astype(np.float32) if m.dense_len else None
            wts = rng.standard_normal(keys.shape).astype(np.float32) if pooled else None
            what = "%s, pooled %d" % (kind, pooled)
            got_rows = run_resolve(fr, ctx, wk, keys, 0, bool(pooled), what=what)
            assert_rows(got_rows, rows, what)
            plain = (wk.infer_pooled(rows, dense, weights=wts) if pooled else wk.infer(rows, dense)).view(np.uint32)
            got = (wk.infer_pooled_keyed(keys, dense, wts) if pooled else wk.infer_keyed(keys, dense)).view(np.uint32)
            assert np.array_equal(got, plain), what
            wk._load_keys(keys, keys.shape[1], dense)      # (the weights are still in the pinned buffer)
            wk.submit_keyed(B, pooled)
            gi, gs = wk._topk_host(B, K, off)
            R.assert_same((gi, gs.view(np.uint32)), R.reference(plain, K, off), "ranking after submit_keyed, " + what)
            out.append((what, got_rows, plain, (gi, gs.view(np.uint32))))
            wk.close()
        finally:
            ctx.close()
    return out


# ---- 7. misses ---------------------------------------------------------------------------------------------------------------------------------------

def check_misses(fr, device):
    """The counter equals the reference's count over several batches, per worker; reading without reset keeps it, reset clears it; a forgotten key
    and a -1 are no misses."""
    rng = np.random.default_rng(7700)
    m, ctx = Q.context(fr, device, "C_bank")
    try:
        C = m.idx_cols
        sp = Spaces(fr, ctx, m)
        sp.cycle(rng)
        pools = Pools(rng, sp)
        wk, other = fr.Worker(ctx, 4097), fr.Worker(ctx, 64)
        assert wk.key_misses() == 0                                                  # before the first resolve
        total = 0
        for B in (1, 64, 301, 4097, 65):
            keys, rows, misses = pools.draw(rng, B, word_cols(C, 0))
            assert_rows(run_resolve(fr, ctx, wk, keys), rows, "batch %d" % B)
            total += misses
            assert wk.key_misses(reset=False) == total
        assert total > 0 and wk.key_misses() == total and wk.key_misses() == 0 and other.key_misses() == 0
        col = next(c for c in range(C) if sp.mode[c] == fr.KEYS_MAPPED)
        known = int(pools.keys[col][0])
        sp.put(col, [known], [sp.miss[col]])                                          # forgotten: still found
        keys = np.full((3, C), -1, np.int64)
        keys[0, col], keys[1, col] = known, 0x0123456789abcdef
        got = run_resolve(fr, ctx, other, keys)
        assert got[0, col] == sp.miss[col] == got[1, col] and got[2, col] == -1
        assert other.key_misses() == 1 and wk.key_misses() == 0
        wk.close()
        other.close()
    finally:
        ctx.close()


# ---- 8. errors and state -----------------------------------------------------------------------------------------------------------------------------

def check_errors(fr, device):
    L = fr.lib()
    rng = np.random.default_rng(7800)
    INV, ST, OK = fr.FR_ERR_INVALID, fr.FR_ERR_STATE, fr.FR_OK
    m, ctx = Q.context(fr, device, "narrow")
    try:
        C, h = m.idx_cols, ctx._h
        old = fr.Worker(ctx, 64)                                                        # a worker older than the key space
        assert old.key_rows() is None and ctx.key_space(1) == (fr.KEYS_ROWS, 0, 0, 0, NO_ROW)
        idx = Q.valid_rows(rng, m, 64).view(np.int32)
        before = old.infer(idx).view(np.uint32)
        sks = lambda ctx_h=h, col=2, mode=fr.KEYS_MAPPED, seed=1, max_keys=8, miss=-1: L.fr_ctx_set_key_space(ctx_h, col, mode, seed, max_keys, miss)
        for bad in (dict(ctx_h=None), dict(col=-1), dict(col=C), dict(mode=3), dict(mode=-1), dict(max_keys=0), dict(max_keys=-5), dict(max_keys=2 ** 30 + 1),
                    dict(miss=-2), dict(miss=90), dict(miss=NO_ROW - 1)):
            assert sks(**bad) == INV, bad
        assert ctx.key_space(2)[0] == fr.KEYS_ROWS                                      # nothing changed
        d_idx, d_rec = fr.DeviceBuffer.from_numpy(ctx, idx), fr.DeviceBuffer(ctx, 64 * m.record_len * 4)
        old.gather_only(64, d_idx, None, d_rec)
        assert sks() == ST and "in flight" in L.fr_last_error().decode()                # work in flight
        old.sync()
        assert sks(miss=89) == OK and sks(miss=NO_ROW) == OK and sks(mode=fr.KEYS_HASHED, max_keys=0, miss=-7) == OK and sks() == OK
        assert ctx.key_space(2) == (fr.KEYS_MAPPED, 1, 8, 0, -1)
        assert L.fr_ctx_key_space(None, 0, None, None, None, None, None) == INV and L.fr_ctx_key_space(h, C, None, None, None, None, None) == INV
        assert L.fr_ctx_key_space(h, 2, None, None, None, None, None) == OK
        # the older worker: the device form works, the host form does not; every existing entry point is unaffected
        assert L.fr_worker_submit_keyed(old._h, 64, 0) == ST and "after the context's first fr_ctx_set_key_space" in L.fr_last_error().decode()
        assert np.array_equal(old.infer(idx).view(np.uint32), before)
        keys = np.zeros((4, C), np.int64)
        assert np.array_equal(run_resolve(fr, ctx, old, keys)[:, :2], np.zeros((4, 2), np.int32))
        old.close()
        wk = fr.Worker(ctx, 64)
        assert wk.key_rows() is not None and wk.key_rows().size == 64 * C
        # puts
        k8, r4 = np.arange(4, dtype=np.int64), np.zeros(4, np.int32)
        pk, pr = k8.ctypes.data, r4.ctypes.data
        d_k, d_r = fr.DeviceBuffer.from_numpy(ctx, k8), fr.DeviceBuffer.from_numpy(ctx, r4)
        for put, a, b in ((lambda *x: L.fr_ctx_put_keys(h, *x), pk, pr), (lambda *x: L.fr_worker_put_keys(wk._h, *x), d_k.ptr, d_r.ptr)):
            assert put(2, 0, None, None) == OK and put(2, -1, a, b) == INV and put(2, 4, None, b) == INV and put(2, 4, a, None) == INV
            assert put(C, 4, a, b) == INV and put(-1, 4, a, b) == INV
            assert put(0, 4, a, b) == ST and "FR_KEYS_MAPPED" in L.fr_last_error().decode()     # a column without a map
        assert L.fr_ctx_put_keys(None, 2, 4, pk, pr) == INV and L.fr_worker_put_keys(None, 2, 4, d_k.ptr, d_r.ptr) == INV
        wk.sync()
        assert ctx.key_space(2)[3] == 0                                                 # nothing was enqueued by any of them
        # resolve
        n_out = 64 * 80
        d_keys = fr.DeviceBuffer.from_numpy(ctx, np.zeros(n_out, np.int64))
        d_out = fr.DeviceBuffer.from_numpy(ctx, np.full(n_out, CANARY, np.uint32))

        def rs(w=wk._h, n=64, kind=0, pooled=0, keys=d_keys.ptr, out=d_out.ptr):
            return L.fr_worker_resolve_keys_device(w, n, kind, pooled, keys, out)

        for bad in (dict(w=None), dict(n=0), dict(n=65), dict(n=-1), dict(kind=3), dict(kind=-1), dict(pooled=2), dict(pooled=-1), dict(keys=None), dict(out=None),
                    dict(keys=d_keys.ptr.value + 4)):
            assert rs(**bad) == INV, bad
        assert rs(kind=1) == ST and rs(kind=2) == ST and "fr_ctx_set_request_columns" in L.fr_last_error().decode()   # no split
        assert rs(pooled=1) == ST and "fr_ctx_set_pooling" in L.fr_last_error().decode()                              # no pooling
        assert L.fr_worker_submit_keyed(wk._h, 64, 1) == ST and L.fr_worker_submit_keyed(wk._h, 64, 3) == INV and L.fr_worker_submit_keyed(wk._h, 65, 0) == INV
        assert L.fr_worker_submit_keyed(None, 64, 0) == INV
        wk.sync()
        assert (d_out.download(np.uint32, n_out) == CANARY).all(), "a refused call wrote its output"
        # key spaces survive set_pooling / set_request_columns; the widths follow both
        ctx.put_keys(2, [10, 20], [1, 2])
        ctx.set_pooling(np.array([2, 1, 3], np.int32))
        ctx.set_request_columns(np.array([1, 0, 1], np.int32))
        assert ctx.key_space(2) == (fr.KEYS_MAPPED, 1, 8, 2, -1)
        assert rs(n=2 ** 24 + 1, kind=1) == INV and rs(n=65, kind=2) == INV              # (request rows may outnumber max_batch, candidate rows may not)
        assert rs(n=65, kind=1) == OK
        wk.sync()
        pw = fr.Worker(ctx, 64)                                                         # (its buffers hold pooled rows)
        want = {(0, 0): [0, 1, 2], (0, 1): [0, 0, 1, 2, 2, 2], (1, 0): [0, 2], (1, 1): [0, 0, 2, 2, 2], (2, 0): [1], (2, 1): [1]}
        for (kind, pooled), wcol in want.items():
            keys = np.full((3, len(wcol)), 7, np.int64)
            keys[:, [i for i, c in enumerate(wcol) if c == 2]] = [[10], [20], [30]]
            rows = np.full(keys.shape, 7, np.int32)
            rows[:, [i for i, c in enumerate(wcol) if c == 2]] = [[1], [2], [-1]]
            assert_rows(run_resolve(fr, ctx, pw, keys, kind, bool(pooled)), rows, "widths after set_pooling / set_request_columns %s" % ((kind, pooled),))
        ctx.set_pooling(np.array([1, 1, 4], np.int32))                                  # the tables follow a change of the pooling
        keys = np.full((2, 6), -1, np.int64)
        keys[:, 5] = [20, 10]
        assert list(run_resolve(fr, ctx, pw, keys, 0, True)[:, 5]) == [2, 1]
        ctx.set_request_columns(np.array([1, 1, 0], np.int32))                          # ... and of the split
        assert rs(w=pw._h, n=4, kind=1, pooled=1) == OK
        pw.sync()
        keys = np.full((2, 4), -1, np.int64)
        keys[:, 0] = [10, 30]
        assert list(run_resolve(fr, ctx, pw, keys, 2, True)[:, 0]) == [1, -1]
        pw.close()
        wk.close()
        for b in (d_idx, d_rec, d_k, d_r, d_keys, d_out):
            b.free()
    finally:
        ctx.close()
    m, ctx = Q.context(fr, device, "narrow")                                            # a key array reaching 4000 MiB
    try:
        ctx.set_pooling(np.array([64, 64, 1], np.int32))
        ctx.set_request_columns(np.array([1, 1, 0], np.int32))
        wk = fr.Worker(ctx, 16)
        d = fr.DeviceBuffer.from_numpy(ctx, np.zeros(16 * 129, np.int64))
        assert L.fr_worker_resolve_keys_device(wk._h, 2 ** 24, 1, 1, d.ptr, d.ptr) == INV and "4000 MiB" in L.fr_last_error().decode()   # 2^24 x 128 keys: 16 GiB
        wk.sync()
        d.free()
        wk.close()
    finally:
        ctx.close()
    c0 = fr.Context(Q.model(fr, "narrow"), device=device, shard_rank=0, n_shards=2)   # a sharded context
    try:
        assert L.fr_ctx_set_key_space(c0._h, 0, fr.KEYS_HASHED, 1, 0, 0) == ST and "sharded" in L.fr_last_error().decode()
        c0.fill_tables(fr.FILL_HASH, 7)
        w0 = fr.Worker(c0, 16)
        d = fr.DeviceBuffer.from_numpy(c0, np.zeros(64, np.int64))
        assert L.fr_worker_resolve_keys_device(w0._h, 4, 0, 0, d.ptr, d.ptr) == ST
        w0.sync()
        d.free()
        w0.close()
    finally:
        c0.close()


# ---- 9. the companion code object --------------------------------------------------------------------------------------------------------------------

KEYS_LAUNCHERS = ["fr_key_fill_launch", "fr_key_put_launch", "fr_key_resolve_launch"]


def check_companion(fr):
    """libfleetrec_keys.so (companion.check_companion)"""
    import companion
    companion.check_companion(fr, KEYS_LIB, KEYS_LAUNCHERS, {"key_fill_kernel": 1, "key_put_kernel": 1, "key_resolve_kernel": 2}, "key_", (fr.LIB_PATH,))


# ---- 10. lifetime --------------------------------------------------------------------------------------------------------------------------------------

def lifetime_cycle(fr, m, device, rng):
    """Key spaces set, replaced and dropped, workers and a context coming and going around them; everything is released with close()."""
    import lifetime
    C, B = m.idx_cols, lifetime.B
    ctx = lifetime.make_ctx(fr, m, device)
    early = fr.Worker(ctx, B)
    for max_keys in (4, 300, 4):                                                  # a map replaced by a larger and by a smaller one
        ctx.set_key_space(0, fr.KEYS_MAPPED, 9, max_keys, 0)
        ctx.put_keys(0, [5, 6, 7], [1, 2, 3])                                     # (its staging)
        wk = fr.Worker(ctx, B)
        keys = lifetime.rows_of(rng, m, B).astype(np.int64)
        keys[:, 0] = rng.integers(5, 9, size=B)
        rows = keys.astype(np.int32)
        rows[:, 0] = np.array([1, 2, 3, 0], np.int32)[keys[:, 0] - 5]
        assert np.array_equal(wk.infer_keyed(keys, lifetime.dense_of(np.random.default_rng(1), m, B)), wk.infer(rows, lifetime.dense_of(np.random.default_rng(1), m, B)))
        assert wk.key_misses() == int((keys[:, 0] == 8).sum())
        wk.close()
    ctx.set_key_space(C - 1, fr.KEYS_HASHED, 4)
    ctx.set_key_space(0, fr.KEYS_ROWS)                                            # dropped
    d, o = fr.DeviceBuffer.from_numpy(ctx, np.zeros(B * C, np.int64)), fr.DeviceBuffer(ctx, B * C * 4)
    early.resolve_keys_device(B, d, o)                                            # a worker older than every key space: its miss counter is made here
    early.sync()
    d.free()
    o.free()
    ctx.set_key_space(0, fr.KEYS_MAPPED, 1, 64, -1)                               # a map alive when the context closes, a worker outliving the context
    ctx.close()
    early.close()

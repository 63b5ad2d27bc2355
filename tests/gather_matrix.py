"""The gather matrix (helpers and case tables only; the tests are tests/test_gather_matrix_cpu.py and tests/test_gpu_gather_matrix.py).

Every kernel instantiation of csrc/fr_gather.hip is named by a case below, at the smallest shape that selects it and still meets its edges;
the GPU module runs each case and asserts fr_worker_last_kernel() word for word, the CPU module runs the fp32 cases on the CPU back-end and
checks that the library holds no gather kernel that no case names.  The reference is expected_records(): the record built segment by
segment from the model's segments and the tables the test itself uploaded -- no oracle, no library call.  Every comparison is
np.array_equal over the WHOLE destination allocation: the records sit inside a larger buffer filled with a sentinel NaN pattern, so a
store before the first item, past the last one or into a shard slice's pad columns shows as well.  No tolerance anywhere.

Transport forms of a record float x (finite): bf16 = bf16_round(x) >> 16, e4m3 = e4m3_encode(x * 2^e_x) (tests/gpu_helpers.py); both are
elementwise, so the expected low-precision records are the gather of the converted tables.  Non-finite inputs: lp_expected()."""
import ctypes

import numpy as np

import pooled_helpers as P
from gpu_helpers import bf16_round, e4m3_encode

INDEX_PER_TABLE, INDEX_PER_ITEM, INDEX_PER_BANK = 0, 1, 2
MODES = {"table": INDEX_PER_TABLE, "item": INDEX_PER_ITEM, "bank": INDEX_PER_BANK}
SEG_DENSE = 2
FR_ERR_INDEX_RANGE, FR_ERR_STATE = -5, -6
SENT = 0x7FC01234                       # the sentinel every destination allocation is filled with (a quiet-NaN pattern)
ESZ = {0: 4, 1: 2, 2: 1}                # bytes a record float is stored as: fp32, bf16, e4m3
NP_T = {0: np.uint32, 1: np.uint16, 2: np.uint8}
E_X = 8                                 # X exponent of the e4m3 one-hot cases: N(0, 3) tables x 2^8 saturate in more than half of the values
CPU = -1


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def expected_records(model, tables, idx, dense=None):
    """The record of every item, [B][K] in the tables' element type (float32 tables are taken as their uint32 bits): segment by segment
    from model.segments() -- a TABLE / COPY segment copies `len` elements from column src_col of row idx[b][column of the table] of table
    src, the DENSE segment the request's own floats.  The table's index column is the table (per-table), its bank (per-bank) or 0."""
    idx = np.asarray(idx).reshape(len(idx), -1)
    mode = model.desc.index_mode
    bank_of = model.bank_map()[0] if mode == INDEX_PER_BANK else None
    tables = [None if t is None else _bits(t) for t in tables]
    out = np.empty((idx.shape[0], model.record_len), next(t for t in tables if t is not None).dtype)
    for sg in model.segments():
        dst = slice(sg.rec_offset, sg.rec_offset + sg.len)
        if sg.kind == SEG_DENSE:
            out[:, dst] = _bits(dense)[:, sg.src_col:sg.src_col + sg.len]
        else:
            col = sg.src if mode == INDEX_PER_TABLE else (int(bank_of[sg.src]) if mode == INDEX_PER_BANK else 0)
            out[:, dst] = tables[sg.src][idx[:, col], sg.src_col:sg.src_col + sg.len]
    return out


def transport(x, tp, e_x=0):
    """FINITE float32 values (or their bits) -> what the gather stores for them: the uint32 bits, bf16 halves (RNE), e4m3 bytes of x * 2^e_x."""
    x = np.ascontiguousarray(x)
    x = x.view(np.float32) if x.dtype == np.uint32 else x.astype(np.float32)
    if tp == 0:
        return x.view(np.uint32)
    if tp == 1:
        return (bf16_round(x).view(np.uint32) >> 16).astype(np.uint16)
    with np.errstate(over="ignore"):
        return e4m3_encode(x * np.float32(2.0 ** e_x))


NAN16, NAN8 = 0x7FC0, 0x7F   # what both sides of a comparison carry where the input is a NaN and the output is one too


def lp_expected(bits, tp, e_x=0):
    """uint32 fp32 patterns of ANY class -> (expected bf16 / e4m3 codes, is_nan mask of the inputs).  Finite values and infinities follow
    transport() (bf16: RNE, an overflowing carry gives the infinity, subnormals as IEEE; e4m3: the product in fp32, clamped to +-448, RNE --
    an infinite input or product gives +-448, -0 keeps its sign).  A NaN input has no single expected code: the contract (fr_device.h) is
    that it stays a NaN -- bf16: exponent all ones and a nonzero mantissa, e4m3: code & 0x7F == 0x7F; canon() maps such outputs to one code."""
    bits = np.ascontiguousarray(bits, np.uint32)
    nan = ((bits & 0x7F800000) == 0x7F800000) & ((bits & 0x007FFFFF) != 0)
    want = transport(np.where(nan, np.uint32(0), bits), tp, e_x)
    want[nan] = NAN16 if tp == 1 else NAN8
    return want, nan


def canon(got, nan, tp):
    """The device's codes with every NaN code at a NaN input replaced by the one lp_expected() carries there (any other code stays and fails)."""
    got = np.array(got)
    is_nan = (((got & 0x7F80) == 0x7F80) & ((got & 0x007F) != 0)) if tp == 1 else ((got & 0x7F) == 0x7F)
    got[nan & is_nan] = NAN16 if tp == 1 else NAN8
    return got


LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def exhaustive_bits():
    """uint32 [6144][64]: every fp32 pattern (h << 16) | l, h over all 65536 upper halves, l over LOW_HALVES: every bf16 tie with its two
    neighbours, every e4m3 code and midpoint at any power-of-two scale, +-0, +-inf, 1534 NaN patterns, the fp32 subnormals."""
    h = np.arange(65536, dtype=np.uint32)[:, None] << np.uint32(16)
    return (h | np.array(LOW_HALVES, np.uint32)[None, :]).reshape(6144, 64)


# ---- models ----------------------------------------------------------------------------------------------------------------------------

def _spec(name):
    if name == "narrow":     # 98 words (one whole wave and a partial one): widths 4 .. 64, a dense block in the middle, a COPY pad, two tables per bank
        dims = [4, 8, 16, 32, 64, 8, 4, 4, 64, 64, 32, 16, 64]
        rows = [50, 1000, 333, 77, 2048, 9, 100, 5000, 300, 400, 700, 64, 900]
        return {"name": "gm_narrow", "tables": [{"dim": d, "rows": r, "class": "HBM", "bank": t // 2} for t, (d, r) in enumerate(zip(dims, rows))],
                "dense_len": 8, "dense_at": 3, "pad": [{"after_table": 5, "copy_of": 4, "col": 8}], "fc": [64, 32, 32]}
    if name == "wide":       # 530 words, 51 tables in 26 banks: the planner deals 8 groups
        dims = [64, 32, 64, 16, 64, 8, 64, 4] * 6 + [64] * 3
        return {"name": "gm_wide", "tables": [{"dim": d, "rows": 37 + 11 * (t % 9), "class": "HBM", "bank": t // 2} for t, d in enumerate(dims)],
                "dense_len": 28, "dense_at": 25, "pad": [{"after_table": 40, "copy_of": 2, "col": 12}], "fc": [64, 32, 32]}
    if name == "big":        # 1920 words: the widest record of 64-float tables the planner still deals in 8 groups of <= 256 words
        return {"name": "gm_big", "tables": [{"dim": 64, "rows": 31 + t % 13} for t in range(120)], "fc": [64, 32, 32]}
    if name == "noplan":     # 2112 words: 264 per group, wider than a workgroup -- no plan
        return {"name": "gm_noplan", "tables": [{"dim": 64, "rows": 31 + t % 13} for t in range(132)], "fc": [64, 32, 32]}
    if name == "shards":     # 4800 floats; two shards of >= 512 words whose lengths differ: the shorter slice has pad columns
        dims = [64] * 33 + [32] * 2 + [64] * 41
        return {"name": "gm_shards", "tables": [{"dim": d, "rows": 30 + 7 * (t % 11)} for t, d in enumerate(dims)], "fc": [64, 32, 32]}
    if name == "exh16":      # the exhaustive rounding table alone: 16 words (the narrow kernel at any batch)
        return {"name": "gm_exh16", "tables": [{"dim": 64, "rows": 6144}], "fc": [64, 32, 32]}
    if name == "exh512":     # 32 copies of it, each rolled by its table number: 512 words with a plan (the stream kernel from batch 1024 on)
        return {"name": "gm_exh512", "tables": [{"dim": 64, "rows": 6144} for _ in range(32)], "fc": [64, 32, 32]}
    if name == "exh256":     # four copies in four banks under an FC chain whose large-batch gather reads the operand-type bank image
        return {"name": "gm_exh256", "tables": [{"dim": 64, "rows": 6144} for _ in range(4)], "fc": [2048, 512, 256]}
    raise KeyError(name)


def make_model(fr, name, mode="table"):
    if name == "mixed":
        return P.mixed_spec_model(fr, MODES[mode])
    return fr.Model.from_spec(_spec(name)).clone(index_mode=MODES[mode])


# ---- the one-hot matrix ----------------------------------------------------------------------------------------------------------------
# id, model, index mode, batches (prefixes of one index set), transport (0 fp32, 1 bf16, 2 e4m3), gather variant, the kernel
# fr_worker_last_kernel() must report; plan: True = fr_ctx_gather_groups must succeed, False = it must refuse; shards = sharded contexts
# (every rank is run); big = records past 200 MiB (GPU only, compared block by block).

def _c(id, model, mode, batches, tp, kernel, variant="word", plan=None, shards=1, big=False):
    return dict(id=id, model=model, mode=mode, batches=tuple(batches), tp=tp, kernel=kernel, variant=variant, plan=plan, shards=shards, big=big)


_M3 = ("table", "bank", "item")
CASES = (
    # gather_pack_kernel<4, TP>: batch < 2048 of a narrow record; 1, 5 and 2047 items against 4 items per thread
    [_c("pack4-tp%d" % tp, "narrow", _M3[tp], (1, 5, 2047), tp, "gather_pack_kernel<4, %d>" % tp) for tp in range(3)]
    # gather_pack_kernel<8, TP>: the same record from batch 2048 on
    + [_c("pack8-tp%d" % tp, "narrow", _M3[(tp + 1) % 3], (2048, 2053), tp, "gather_pack_kernel<8, %d>" % tp) for tp in range(3)]
    # gather_pack_stream_kernel<4, 2, TP, 16, false>: >= 512 words with a plan, batch >= 1024.  A workgroup walks 2 chunks of 4 items: the
    # batch ends on a chunk (1024), inside a workgroup's first chunk (1027), inside its second (1029), on a whole workgroup (1032)
    + [_c("stream16-tp%d" % tp, "wide", _M3[(tp + 2) % 3], (1024, 1027, 1029, 1032), tp, "gather_pack_stream_kernel<4, 2, %d, 16, false>" % tp, plan=True)
       for tp in range(3)]
    # ... its write-back store form: records past 200 MiB (209,715,200 bytes): 7003 x 30720, 14003 x 15360, 27503 x 7680 bytes
    + [_c("stream0-tp%d" % tp, "big", "table", (b,), tp, "gather_pack_stream_kernel<4, 2, %d, 0, false>" % tp, plan=True, big=True)
       for tp, b in ((0, 7003), (1, 14003), (2, 27503))]
    # gather_pack_xcd_kernel<4, TP, 0>: the one-chunk-per-workgroup variant on the same record
    + [_c("xcd-tp%d" % tp, "wide", _M3[tp], (1027,), tp, "gather_pack_xcd_kernel<4, %d, 0>" % tp, variant="one_chunk", plan=True) for tp in range(3)]
    # gather_tile_kernel<DEDUP>: a ragged batch; column 0 holds <= 8 distinct rows (leaders, duplicates and hash-slot collisions in one
    # wave), another column all-distinct rows (tile_idx)
    + [_c("tile-plain", "narrow", "table", (203,), 0, "gather_tile_kernel<false>", variant="tile"),
       _c("tile-dedup", "narrow", "table", (203,), 0, "gather_tile_kernel<true>", variant="dedup"),
       _c("tile-dedup-bank", "narrow", "bank", (203,), 0, "gather_tile_kernel<true>", variant="dedup")]
    # no plan: a record wider than 8 x 256 words at a batch that would take the XCD form falls back to gather_pack_kernel
    + [_c("noplan", "noplan", "table", (1027,), 0, "gather_pack_kernel<4, 0>", plan=False)]
    # sharded contexts: the destination is [batch][padded slice], wider than the shorter shard's own words
    + [_c("shards-tp%d" % tp, "shards", "table", (1027,), tp, "gather_pack_stream_kernel<4, 2, %d, 16, false>" % tp, plan=True, shards=2) for tp in range(3)]
)
VARIANTS = {"word": 0, "tile": 1, "dedup": 2, "one_chunk": 4}   # fr.GATHER_WORD_MAJOR / ITEM_TILE / ITEM_TILE_DEDUP / WORD_MAJOR_ONE_CHUNK


def onehot_kernel_for(n_words, out_words, batch, tp, variant, has_plan):
    """gather_launch / gather_launch_xcd restated: n_words the context's own record words, out_words the destination's words per item."""
    if variant in ("tile", "dedup"):
        return "gather_tile_kernel<%s>" % ("true" if variant == "dedup" else "false")
    if n_words >= 512 and batch >= 1024 and (has_plan or (n_words + 7) // 8 <= 256):
        if variant == "one_chunk":
            return "gather_pack_xcd_kernel<4, %d, 0>" % tp
        return "gather_pack_stream_kernel<4, 2, %d, %d, false>" % (tp, 16 if batch * out_words * 4 * ESZ[tp] <= 200 << 20 else 0)
    return "gather_pack_kernel<%d, %d>" % (8 if batch >= 2048 else 4, tp)


def case_seed(case):
    return 9000 + sum(map(ord, case["id"]))


def case_data(model, case):
    """-> (tables, idx int32 [Bmax][cols], dense float32 [Bmax][dense_len] or None).  fp32 cases carry random BIT patterns (a bit copy must
    keep every one of them), the low-precision cases finite values N(0, 3); index 0 in item 0 and the last row in item 1 of every column."""
    rng = np.random.default_rng(case_seed(case))
    B = max(case["batches"])
    tabs = model.tables()
    if case["tp"] == 0:
        tables = [rng.integers(0, 2 ** 32, size=(int(t.rows), t.dim), dtype=np.uint32) for t in tabs]
    else:
        tables = [(3.0 * rng.standard_normal((int(t.rows), t.dim))).astype(np.float32) for t in tabs]
    ranges = model.index_ranges()
    idx = (rng.random((B, len(ranges))) * ranges[None, :]).astype(np.int32)
    if case["variant"] in ("tile", "dedup"):
        idx[:, 0] = rng.integers(0, min(8, int(ranges[0])), size=B)
        c = next(c for c in range(1, len(ranges)) if ranges[c] >= B)
        idx[:, c] = rng.permutation(int(ranges[c]))[:B]
    idx[0] = 0
    if B > 1:
        idx[1] = ranges - 1
    dense = (3.0 * rng.standard_normal((B, model.dense_len))).astype(np.float32) if model.dense_len else None
    return tables, idx, dense


# ---- destinations with room on either side ---------------------------------------------------------------------------------------------

def _up(n, a):
    return (n + a - 1) // a * a


class Guarded:
    """A destination of B items x `stride` bytes inside a larger device allocation filled with SENT: at least two items' stride in front
    (a store before the first item) and 16 items' behind (two chunks of the widest kernel: 8 items per thread), both 256-byte multiples."""

    def __init__(self, fr, ctx, B, stride):
        self.fr, self.ctx, self.B, self.stride = fr, ctx, B, stride
        self.pre, self.post = _up(2 * stride, 256), _up(16 * stride, 256)
        self.total = self.pre + B * stride + self.post
        assert self.total % 4 == 0
        self.buf = fr.DeviceBuffer(ctx, self.total)
        self.fill()

    def fill(self):
        self.buf.upload(np.full(self.total // 4, SENT, np.uint32))

    @property
    def ptr(self):
        return self.buf.ptr.value + self.pre

    def check(self, rows_fn, own, block=1024, skip=None):
        """Download the allocation: both margins and every item's bytes past `own` still hold the sentinel, and items [b0, b0 + n) hold
        rows_fn(b0, n) (an array of n x own bytes in any element type), block by block.  skip: bool [B][own bytes] -- bytes of an
        offending lookup, which belong to no reference."""
        got = self.buf.download(np.uint8, self.total)
        sent = np.full(max(self.pre, self.post) // 4, SENT, np.uint32).view(np.uint8)
        assert np.array_equal(got[:self.pre], sent[:self.pre]), "the gather wrote in front of the records"
        assert np.array_equal(got[self.total - self.post:], sent[:self.post]), "the gather wrote past the records"
        for b0 in range(0, self.B, block):
            n = min(block, self.B - b0)
            rows = got[self.pre + b0 * self.stride:self.pre + (b0 + n) * self.stride].reshape(n, self.stride)
            want = np.ascontiguousarray(rows_fn(b0, n)).view(np.uint8).reshape(n, own)
            have = rows[:, :own]
            if skip is not None:
                keep = ~skip[b0:b0 + n]
                have, want = have[keep], want[keep]
            assert np.array_equal(have, want), "items %d..%d: %d bytes differ" % (b0, b0 + n - 1, int((have != want).sum()))
            if own < self.stride:
                pad = np.ascontiguousarray(rows[:, own:]).view(np.uint32)
                assert np.array_equal(pad, np.full(pad.shape, SENT, np.uint32)), "a slice's pad columns were written"

    def free(self):
        self.buf.free()


def _raises_index_range(fr, fn):
    try:
        fn()
    except fr.FleetRecError as e:
        assert e.status == FR_ERR_INDEX_RANGE, e
        return
    raise AssertionError("an out-of-range index was not reported")


def offending_bytes(fr, model, B, item, col, lo, own_floats, esz):
    """bool [B][own bytes]: the bytes of item `item` that index column `col` feeds, inside the floats [lo, lo + own_floats) of the record."""
    cols = P.column_of_float(fr, model)[lo:lo + own_floats]
    skip = np.zeros((B, own_floats * esz), bool)
    skip[item] = np.repeat(cols == col, esz)
    return skip


def run_onehot(fr, device, case, assert_kernel=True):
    """One case of CASES on `device` (CPU = the CPU back-end: fp32 only, no kernel names): every batch into a guarded destination, then
    (not for the 200 MiB cases) an out-of-range index in item 0 and in the last item, and a clean gather after each.  -> seconds per batch
    spent between the launch and the end of the sync (for the summary's figures)."""
    import time
    m = make_model(fr, case["model"], case["mode"])
    tables, idx, dense = case_data(m, case)
    tp, esz = case["tp"], ESZ[case["tp"]]
    e_x = E_X if tp == 2 else 0
    lp_tables = [transport(t, tp, e_x) for t in tables]
    lp_dense = None if dense is None else transport(dense, tp, e_x)
    n_sh = case["shards"]
    offs, lens, F = m.shard_plan(n_sh) if n_sh > 1 else ([0], [m.record_len], m.record_len)
    if n_sh > 1:
        assert min(lens) // 4 >= 512 and min(lens) < F
    ranges = m.index_ranges()
    times = []
    for rank in range(n_sh):
        lo, own = offs[rank], lens[rank]
        ctx = fr.Context(m, device=device, shard_rank=rank, n_shards=n_sh)
        try:
            for sg in m.segments():
                if sg.kind != SEG_DENSE and (n_sh == 1 or lo <= sg.rec_offset < lo + own):
                    ctx.upload_table(sg.src, tables[sg.src])
            if tp == 2:
                ctx.set_fp8_act_exponents([e_x, 0, 0, 0])
            if case["plan"] is True and device != CPU:   # (the CPU back-end walks the words and plans nothing)
                st = ctx.gather_groups()   # a lost plan fails here, loudly, instead of taking another kernel
                assert st[0] == 0 and st[8] == own // 4
            elif case["plan"] is False and device != CPU:
                try:
                    ctx.gather_groups()
                    raise AssertionError("a record of %d words has an XCD plan" % (own // 4))
                except fr.FleetRecError as e:
                    assert e.status == FR_ERR_STATE
            if device != CPU:
                ctx.set_gather_variant(VARIANTS[case["variant"]])
            Bmax = max(case["batches"])
            wk = fr.Worker(ctx, Bmax)
            d_idx = fr.DeviceBuffer.from_numpy(ctx, idx)
            d_dense = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None

            def gather(B, di, dst):
                t0 = time.perf_counter()
                if tp == 0:
                    wk.gather_only(B, di, d_dense, dst.ptr)
                else:
                    wk.gather_slices(B, di, d_dense, dst.ptr, tp)
                name = wk.last_kernel()
                wk.sync()
                times.append((B, time.perf_counter() - t0))
                if assert_kernel:
                    assert name == case["kernel"], (name, case["kernel"])

            def rows_fn(b0, n, _idx=idx):
                return expected_records(m, lp_tables, _idx[b0:b0 + n], None if lp_dense is None else lp_dense[b0:b0 + n])[:, lo:lo + own]

            for B in case["batches"]:
                dst = Guarded(fr, ctx, B, F * esz)
                gather(B, d_idx, dst)
                dst.check(rows_fn, own * esz)
                dst.free()
            if not case["big"]:
                B = Bmax
                dst = Guarded(fr, ctx, B, F * esz)
                cols_here = sorted(set(int(c) for c in P.column_of_float(fr, m)[lo:lo + own] if c >= 0))
                for item, col, val in ((0, cols_here[0], int(ranges[cols_here[0]])), (B - 1, cols_here[-1], 2 ** 30)):
                    bad = idx[:B].copy()
                    bad[item, col] = val
                    d_bad = fr.DeviceBuffer.from_numpy(ctx, bad)
                    dst.fill()
                    _raises_index_range(fr, lambda: gather(B, d_bad, dst))
                    dst.check(lambda b0, n: rows_fn(b0, n, bad.clip(0, ranges[None, :] - 1)), own * esz,
                              skip=offending_bytes(fr, m, B, item, col, lo, own, esz))
                    dst.fill()
                    gather(B, d_idx, dst)      # the flag does not stick: the next good gather on the same worker is clean
                    dst.check(rows_fn, own * esz)
                    d_bad.free()
                dst.free()
            wk.close()
        finally:
            ctx.close()
    return times


# ---- the pooled matrix -----------------------------------------------------------------------------------------------------------------
# kernel -> the bag lengths (cycled over the index columns) that make frk_gather_pooled select it
POOLED_HOTS = {
    "gather_pooled_kernel<4, 2, false>": (1,),
    "gather_pooled_kernel<2, 2, false>": (1, 2, 3),
    "gather_pooled_kernel<2, 4, false>": (1, 3, 4, 5, 7),
    "gather_pooled_kernel<2, 4, true>": (4,),
    "gather_pooled_kernel<2, 8, false>": (1, 2, 5, 8, 9, 15),
    "gather_pooled_kernel<2, 8, true>": (4, 8, 12),
    "gather_pooled_kernel<1, 16, false>": (1, 16, 17, 33, 63, 64),
    "gather_pooled_kernel<1, 16, true>": (4, 16, 20, 64),
}
POOLED_BATCHES = (1, 2, 3, 1029)        # ragged against 1, 2 and 4 items per thread; 1029 items are many chunks


def _pc(kernel, model, mode, batches=POOLED_BATCHES):
    k = kernel[len("gather_pooled_kernel<"):-1].replace(", ", "-")
    return dict(id="pool-%s-%s-%s" % (k, model, mode), kernel=kernel, model=model, mode=mode, batches=tuple(batches), hots=POOLED_HOTS[kernel])


POOLED_CASES = (
    # a record with a plan (8 XCD groups) and the mixed-width model below 64 words (one group), index modes spread over the kernels
    [_pc(k, "wide", ("table", "bank")[i % 2]) for i, k in enumerate(POOLED_HOTS)]
    + [_pc(k, "mixed", ("table", "bank", "item", "bank", "table", "bank", "table", "bank")[i]) for i, k in enumerate(POOLED_HOTS)]
    # no plan on a record wider than one workgroup: one group, blockIdx.y > 0
    + [_pc("gather_pooled_kernel<2, 8, false>", "noplan", "table", (3, 131)), _pc("gather_pooled_kernel<1, 16, true>", "noplan", "table", (3, 131))]
)


def pooled_hots(case, n_cols):
    """The case's bag lengths cycled over the columns; with fewer columns than lengths, the longest ones (the longest bag picks the window)."""
    pat = case["hots"]
    if n_cols < len(pat):
        pat = pat[len(pat) - n_cols:]
    return np.array([pat[c % len(pat)] for c in range(n_cols)], np.int32)


def pooled_kernel_for(hots, aligned=True):
    """frk_gather_pooled's choice restated: window by the longest bag, items per thread, 16-byte index loads when every bag is whole groups of 4."""
    mx = int(max(hots))
    win = 16 if mx >= 16 else 8 if mx >= 8 else 4 if mx >= 4 else 2
    items = 1 if win >= 16 else 2 if mx >= 2 else 4
    wide = aligned and win % 4 == 0 and all(int(h) % 4 == 0 for h in hots)
    return "gather_pooled_kernel<%d, %d, %s>" % (items, win, "true" if wide else "false")


SPECIAL_ROWS = {1: 0x80000000, 2: 0x7FA12345, 3: 0x7F800000, 4: 0xFF800000, 5: 0x00000123}   # -0.0, a signalling NaN with a payload, +-inf, a subnormal


def pooled_data(model, case):
    """-> (tables float32, hots, idx int32 [Bmax][P], dense).  Rows 1 .. 5 of every table hold SPECIAL_ROWS in every float; every other row
    is finite (N(0, 3), with a subnormal and a -0.0 sprinkled in).  A bag takes a special row only as its ONLY non-empty slot (a NaN
    through an add is not in the contract); the patterns by (item + column) % 6: 1 empty first slot, 2 empty last slot, 3 only the last
    slot filled (with a special row for every other such bag), 4 the whole bag empty, 5 a lone special row in a random slot."""
    rng = np.random.default_rng(case_seed(case))
    B = max(case["batches"])
    tables = []
    for t in model.tables():
        a = (3.0 * rng.standard_normal((int(t.rows), t.dim))).astype(np.float32)
        u = a.view(np.uint32)
        u[0, 0], u[-1, -1], u[6, 1] = 0x00000007, 0x80000000, 0x807FFFFF
        for r, v in SPECIAL_ROWS.items():
            u[r, :] = v
        tables.append(a)
    ranges = model.index_ranges()
    assert ranges.min() >= 7
    hots = pooled_hots(case, len(ranges))
    pre = P.prefix_of(hots)
    idx = np.full((B, int(hots.sum())), -1, np.int32)
    for c, h in enumerate(hots):
        fin = np.array([r for r in range(int(ranges[c])) if r not in SPECIAL_ROWS], np.int32)
        bag = fin[rng.integers(0, len(fin), size=(B, h))]
        bag[rng.random((B, h)) < 0.2] = -1
        it = np.arange(B)
        pat = np.where((it < 12) | (it >= B - 4) | (rng.random(B) < 0.3), (it + c) % 6, 0)
        pat[20:22] = 0
        bag[pat == 1, 0] = -1
        bag[pat == 2, h - 1] = -1
        last = fin[rng.integers(0, len(fin), size=B)]
        odd = (it // 6) % 2 == 1
        last[odd] = 1 + rng.integers(0, 5, size=int(odd.sum()))
        bag[pat == 3, :] = -1
        bag[pat == 3, h - 1] = last[pat == 3]
        bag[pat == 4, :] = -1
        bag[pat == 5, :] = -1
        lone = np.flatnonzero(pat == 5)
        bag[lone, rng.integers(0, h, size=len(lone))] = 1 + rng.integers(0, 5, size=len(lone))
        if B > 21:   # index 0 and the last row of every column (both finite rows)
            bag[20, 0], bag[21, 0] = 0, ranges[c] - 1
        idx[:, pre[c]:pre[c] + h] = bag
    dense = (3.0 * rng.standard_normal((B, model.dense_len))).astype(np.float32) if model.dense_len else None
    return tables, hots, idx, dense


def pooled_expected(fr, model, tables, hots, idx, dense):
    return P.expected_from_onehot(fr, model, hots, idx, dense, lambda one: expected_records(model, tables, one, dense))


def run_pooled(fr, device, case, assert_kernel=True):
    """One case of POOLED_CASES on `device`: every batch into a guarded destination; for the 16-byte-index forms the same rows again at a
    device address 4, 8 and 12 bytes past a 16-byte boundary (the narrow form must run, the bits must not change); a slot equal to the row
    count in item 0 and a slot of -2 in the last item, and a clean gather after each."""
    m = make_model(fr, case["model"], case["mode"])
    tables, hots, idx, dense = pooled_data(m, case)
    Bmax = max(case["batches"])
    want = pooled_expected(fr, m, tables, hots, idx, dense)
    K = m.record_len
    ranges = m.index_ranges()
    pre = P.prefix_of(hots)
    ctx = fr.Context(m, device=device)
    try:
        for t, a in enumerate(tables):
            ctx.upload_table(t, a)
        ctx.set_pooling(hots)
        assert ctx.pooled_index_cols == idx.shape[1]
        wk = fr.Worker(ctx, Bmax)
        d_dense = fr.DeviceBuffer.from_numpy(ctx, dense) if dense is not None else None
        wide = case["kernel"].endswith("true>")

        def gather(B, rows, dst, shift=0, kernel=case["kernel"]):
            raw = fr.DeviceBuffer(ctx, rows[:B].nbytes + 256)
            base = _up(raw.ptr.value, 16) + shift
            flat = np.ascontiguousarray(rows[:B])
            fr._check(fr.lib().fr_memcpy_h2d(ctx._h, ctypes.c_void_p(base), flat.ctypes.data_as(ctypes.c_void_p), flat.nbytes))
            try:
                wk.gather_pooled(B, base, d_dense, dst.ptr)
                name = wk.last_kernel()
                wk.sync()
            finally:
                raw.free()
            if assert_kernel:
                assert name == kernel, (name, kernel)

        for B in case["batches"]:
            dst = Guarded(fr, ctx, B, K * 4)
            gather(B, idx, dst)
            dst.check(lambda b0, n: want[b0:b0 + n], K * 4)
            if wide and B == Bmax:
                for shift in (4, 8, 12):
                    dst.fill()
                    gather(B, idx, dst, shift, case["kernel"].replace("true>", "false>"))
                    dst.check(lambda b0, n: want[b0:b0 + n], K * 4)
            dst.free()
        B = Bmax
        dst = Guarded(fr, ctx, B, K * 4)
        col_of = P.column_of_float(fr, m)
        for item, c, val in ((0, 0, int(ranges[0])), (B - 1, len(hots) - 1, -2)):
            bad = idx[:B].copy()
            bad[item, pre[c] + int(hots[c]) - 1] = val
            dst.fill()
            _raises_index_range(fr, lambda: gather(B, bad, dst))
            skip = np.zeros((B, K * 4), bool)
            skip[item] = np.repeat(col_of == c, 4)
            dst.check(lambda b0, n: want[b0:b0 + n], K * 4, skip=skip)
            dst.fill()
            gather(B, idx, dst)
            dst.check(lambda b0, n: want[b0:b0 + n], K * 4)
        dst.free()
        wk.close()
    finally:
        ctx.close()
    return want, hots, idx


# ---- kernels of libfleetrec.so that are neither gather_* kernels (CASES / POOLED_CASES) nor FC-chain kernels (tests/exact_chain.py) ------
# kernel -> "file::test" that runs it.  A new kernel of any kind fails tests/test_gather_matrix_cpu.py until someone decides where it is tested.
COVERED_ELSEWHERE = {
    "fill_table_kernel": "tests/test_gpu_gather.py::test_fill_kernels_match_oracle_content",
    "fill_weights_kernel": "tests/test_gpu_scores.py::test_scores_within_tolerance",
    "pack_weights_q4_kernel": "tests/test_gpu_exact_chain.py::test_exact_case",
    "pack_weights_q8_bf16_kernel": "tests/test_gpu_exact_chain.py::test_exact_wide_weights",
    "pack_weights_q16_fp8_kernel": "tests/test_gpu_exact_chain.py::test_exact_wide_weights",
    "pack_weights_q16h_fp8_kernel": "tests/test_gpu_exact_chain.py::test_exact_case",
    "transpose_records_kernel": "tests/test_gpu_exact_chain.py::test_exact_case",
    "records_to_q8_bf16_kernel": "tests/test_gpu_exact_chain.py::test_exact_case",
    "records_to_q16_fp8_kernel": "tests/test_gpu_exact_chain.py::test_exact_case",
    "stats_kernel": "tests/test_gpu_exact_chain.py::test_fp8_weight_exponent_from_the_weights",
    "convert_rows_lp_kernel<1>": "tests/test_gpu_gather_matrix.py::test_operand_image_rounding_exhaustive",
    "convert_rows_lp_kernel<2>": "tests/test_gpu_gather_matrix.py::test_operand_image_rounding_exhaustive",
    "q4_to_lp_kernel<1>": "tests/test_gpu_sharded.py::test_table_sharded_mode_single_device_emulation",
    "q4_to_lp_kernel<2>": "tests/test_gpu_sharded.py::test_table_sharded_mode_single_device_emulation",
    "transpose_slices_kernel": "tests/test_gpu_sharded.py::test_table_sharded_mode_single_device_emulation",
    "transpose_slices_lp_kernel<1>": "tests/test_gpu_sharded.py::test_table_sharded_mode_single_device_emulation",
    "transpose_slices_lp_kernel<2>": "tests/test_gpu_sharded.py::test_table_sharded_mode_single_device_emulation",
}


def named_kernels():
    return {c["kernel"] for c in CASES} | {c["kernel"] for c in POOLED_CASES}

"""The table-sharded FC path on the integer-valued data of tests/exact_chain.py, bit for bit against the host's restatement (helpers only; the
tests are tests/test_cpu_exact_sharded.py and tests/test_gpu_exact_sharded.py, the checks are stated once here and take the device).

What runs: fr_worker_gather_only / fr_worker_gather_slices on every shard, fr_worker_fc_from_slices[_lp] in the all-gather layout
([G][B][F], items [lo, lo + n)) and in the all-to-all layout ([G][n][F], items [0, n)), fr_worker_calibrate_fp8_slices / _sharded, and the
whole fr_worker_submit_sharded step in both exchange modes.  device = -1: G CPU shard contexts on the in-process host exchange, fp32 only;
device >= 0: G GPU shard contexts of one device on the staged exchange.  On integer-valued data every summation order is exact, so every
comparison is np.array_equal whichever kernels a rank's item count selects; ROWS places the shape edges of the slice re-pack kernels
(fr_fill.hip: transpose_slices_kernel, transpose_slices_lp_kernel<1|2>, q4_to_lp_kernel<1|2>, stats_kernel) on purpose.  The columns of a
slice past its own length (up to the common padded length F) hold NaN patterns in every gathered array the FC entry points are handed."""
import threading

import numpy as np

import exact_chain as E
from gpu_helpers import bf16_round, e4m3_decode_table, e4m3_encode

CPU = -1
SEG_DENSE = 2
POOL = 256   # items of a model's pool (exact_chain.make_data): a row's batch is drawn from it, distinct while it lasts

# Each row: the smallest shape that reaches its edge.  `plan` states what Model.shard_plan gives for it (asserted by the CPU test, so that a planner
# change cannot move a row off its edge): off4 / len16 = the residues of the slices' first record word mod 4 and of their lengths in words mod 16,
# items = the ranks' item counts, min_len = the shortest slice in floats, F = the padded slice length, dense_only = (rank, floats) of a shard without
# a table.  `mutants` names the simulated bugs (test_cpu_exact_sharded.py) whose edge the row targets.
ROWS = [
    dict(id="a", model="A352", G=3, B=77, precs=("f32", "bf16", "fp8"),
         edge="slice word offsets = 0, 2 (mod 4); lengths = 0, 10, 14 (mod 16) words; items 26/26/25, so item0 = 26 and 52",
         plan=dict(off4=[0, 2], len16=[0, 10, 14], items=[26, 26, 25], F=128), mutants=("first_word", "last_word", "item0")),
    dict(id="b", model="B880", G=7, B=100, precs=("f32", "bf16", "fp8"),
         edge="offsets hit all four residues mod 4 (bf16 pairs and e4m3 quads straddle shards); the dense block inside a slice",
         plan=dict(off4=[0, 1, 2, 3], dense_inside=True, F=136), mutants=("first_word", "last_word", "item0", "bf16_pair")),
    dict(id="c", model="C", G=8, B=301, precs=("f32", "bf16", "fp8"), edge="Model-C geometry; uneven split (38 x 5, 37 x 3); F = 556",
         plan=dict(F=556, items=[38, 38, 38, 38, 38, 37, 37, 37]), mutants=("first_word", "last_word", "item0", "bf16_pair")),
    dict(id="d", model="C", G=70, B=75, precs=("f32", "fp8"),
         edge="two launches of the 64-shard slice table; one or two items per rank; a plan that held empty shards before the planner fix; "
              "the exchange serves at most 64 ranks, so fr_comm_init_all refuses this G and the step is not run",
         plan=dict(min_len=4, F=128, off4=[0, 1, 2, 3]), mutants=("first_word", "shard_order")),
    dict(id="e", model="P", G=5, B=33, precs=("f32", "fp8"), refused=("bf16",),
         edge="K = 4200, K % 64 = 40: the fp8 image's zero rows past K / 16 and a partly covered last element row; bf16 refuses this K",
         plan=dict(F=892, k_mod_64=40), mutants=("first_word", "last_word", "item0", "fp8_pad")),
    dict(id="f", model="A352", G=2, B=1, precs=("f32", "bf16", "fp8"), edge="rank 1 has no item; ldm = 32 around one item",
         plan=dict(items=[1, 0], F=232), mutants=("first_word", "last_word")),
    dict(id="g", model="B880", G=24, B=50, precs=("f32", "bf16"),
         edge="a 4-float slice (one record word); a shard of the dense block alone, which holds no table and is loaded by upload",
         plan=dict(min_len=4, dense_only=(12, 16), off4=[0, 1, 2, 3], F=128), mutants=("first_word", "item0", "bf16_pair")),
    dict(id="h", model="A352", G=6, B=64, precs=("f32",), edge="the smallest plan that had an empty shard before the planner fix",
         plan=dict(min_len=4, lens=[48, 72, 128, 4, 48, 52]), mutants=("first_word", "last_word", "item0")),
    dict(id="i", model="C", G=2, B=8190, precs=("f32", "bf16", "fp8"), width=1, heavy=True,
         edge="n_items = 4095, ldm 4096, chain width 1: the GEMM-tile kernels fed by the slice transposes",
         plan=dict(items=[4095, 4095], F=2012),
         # what fr_worker_last_kernel names after fc_layer_only(4095, l), l = 0..3 (read from a run on an MI355X)
         layers={"f32": ["fc_lp_gemm_kernel<0, 2, 128, 2, 8, 32>", "fc_lp_gemm_kernel<0, 1, 64, 2, 8, 32>", "fc_lp_gemm_kernel<0, 1, 64, 2, 8, 32>", E.PIPE % (4, 0)],
                 "bf16": ["fc_pp_gemm_n128_kernel<1, 2>", "fc_lp_gemm_kernel<1, 1, 64, 4, 8, 32>", "fc_lp_gemm_out_kernel<1, 2>", E.PIPE % (4, 1)],
                 "fp8": ["fc_pp_gemm_n128_kernel<2, 2>", "fc_lp_gemm_kernel<2, 1, 64, 2, 8, 32>", "fc_lp_gemm_out_kernel<2, 2>", E.PIPE % (4, 2)]},
         mutants=("first_word", "last_word", "item0")),
]
MAX_RANKS = 64   # fr_comm_init_all serves at most this many ranks (fr_comm.cpp)
CELLS = [(row, p) for row in ROWS for p in row["precs"]]
CELL_IDS = ["%s-%s" % (row["id"], p) for row, p in CELLS]


def item_range(rank, world, n):
    import importlib
    return importlib.import_module("fleetrec_amd.dist").item_range(rank, world, n)   # (the package is loaded by the `fr` fixture)


def assemble_records(gathered, offs, lens, K):
    import importlib
    return importlib.import_module("fleetrec_amd.dist").assemble_records(gathered, offs, lens, K)


def row(rid):
    return next(r for r in ROWS if r["id"] == rid)


def precision(fr, name):
    return {"f32": fr.FC_FP32, "bf16": fr.FC_BF16, "fp8": fr.FC_FP8}[name]


def same(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
    assert not bad.any(), "%s: %d of %d items differ, first %s: got %r want %r" % (
        what, int(bad.sum()), bad.size, np.flatnonzero(bad)[:8].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


# ---- data: one model, one pool and one expectation per model name, shared by every test that needs them and never written to ----------------
_models, _expect = {}, {}


def model_data(fr, name):
    """-> (model, data, pool records float32 [POOL][K]) of an exact_chain model."""
    if name not in _models:
        sp = E.model_spec(name)
        data = E.make_data(sp, E.model_seed(name), n_pool=POOL)
        m = fr.Model.from_spec(sp)
        rec = E.records(m, data, data["idx"], data["dense"])
        rec.setflags(write=False)
        _models[name] = (m, data, rec)
    return _models[name]


def selection(r):
    """Which pool items make up the row's batch: distinct while the pool lasts, then drawn again."""
    rng = np.random.default_rng(4000 + sum(map(ord, r["id"] + r["model"])))
    sel = rng.permutation(POOL)
    if r["B"] > POOL:
        sel = np.concatenate([sel, rng.integers(0, POOL, size=r["B"] - POOL)])
    return sel[:r["B"]]


def batch(fr, r):
    """-> (model, data, idx, dense, records) of the row's batch."""
    m, data, pool = model_data(fr, r["model"])
    sel = selection(r)
    return m, data, data["idx"][sel], (data["dense"][sel] if data["dense"] is not None else None), pool[sel]


def expect(fr, r, prec):
    """The row's exact scores in `prec` -> (scores [B], act_exp, w_exp); the premise and (from 32 items on) the rounding witnesses are asserted first.
    A score depends on its own item and, in fp8, on the batch's activation maxima only, so the chain is restated once per distinct pool item."""
    key = (r["id"], prec)
    if key not in _expect:
        _, data, pool = model_data(fr, r["model"])
        u, inv = np.unique(selection(r), return_inverse=True)
        rec, ws = pool[u], data["ws"]
        ae = we = None
        if prec == "fp8":
            ae, we = E.act_exponents(rec, ws), E.w_exponents(ws)   # over the whole batch
        E.premise(prec, rec, ws, ae, we)
        if prec != "f32" and len(u) >= 32:
            for l, (inexact, ties) in enumerate(E.rounding_witnesses(prec, rec, ws, ae, we)):
                assert inexact > 0 and ties > 0, (r["id"], prec, l, inexact, ties)
        want = E.expected(prec, rec, ws, ae, we)[inv]
        want.setflags(write=False)
        _expect[key] = (want, ae, we)
    return _expect[key]


def plan_facts(m, r):
    """What a row's `plan` is compared with, from Model.shard_plan."""
    offs, lens, F = m.shard_plan(r["G"])
    segs = m.segments()
    kinds = [[s.kind for s in segs if offs[g] <= s.rec_offset < offs[g] + lens[g]] for g in range(r["G"])]
    dense_only = [(g, lens[g]) for g in range(r["G"]) if kinds[g] and all(k == SEG_DENSE for k in kinds[g])]
    return dict(off4=sorted(set(o // 4 % 4 for o in offs)), len16=sorted(set(l // 4 % 16 for l in lens)), F=F, min_len=min(lens), lens=lens,
                items=[hi - lo for lo, hi in (item_range(g, r["G"], r["B"]) for g in range(r["G"]))],
                dense_only=dense_only[0] if dense_only else None, dense_inside=any(SEG_DENSE in k and len(set(k)) > 1 for k in kinds),
                k_mod_64=m.record_len % 64)


def held_tables(m, off, ln):
    return sorted(set(s.src for s in m.segments() if s.kind != SEG_DENSE and off <= s.rec_offset < off + ln))


def pad_nan(gathered, lens):
    """The columns past each slice's own length -> NaN patterns of the array's type (float32 NaN, bf16 0x7FC0, e4m3 0x7F)."""
    fill = {np.dtype(np.float32): np.nan, np.dtype(np.uint16): 0x7FC0, np.dtype(np.uint8): 0x7F}[gathered.dtype]
    for g, ln in enumerate(lens):
        gathered[g, :, ln:] = fill
    return gathered


def host_gathered(rec, offs, lens, F):
    """[G][B][F] float32: every shard's slice of the records, NaN past its length (what the shards' gathers deliver, restated)."""
    out = np.full((len(offs), rec.shape[0], F), np.nan, np.float32)
    for g, (o, ln) in enumerate(zip(offs, lens)):
        out[g, :, :ln] = rec[:, o:o + ln]
    return out


def transported(prec, sl, e_x):
    """The wire form of fp32 slice values: bf16 bits (RNE) or e4m3 bytes of the value x 2^e_x."""
    if prec == "bf16":
        return (bf16_round(sl).view(np.uint32) >> 16).astype(np.uint16)
    return e4m3_encode(np.asarray(sl, np.float32) * np.float32(2.0 ** e_x))


# ---- the job: G shard contexts of one device, loaded by upload alone ------------------------------------------------------------------------
class Job:
    def __init__(self, fr, device, r, prec, tables=None, comms=False):
        self.fr, self.device, self.row, self.prec, self.G, self.B = fr, device, r, prec, r["G"], r["B"]
        self.m, self.data, self.idx, self.dense, self.rec = batch(fr, r)
        self.offs, self.lens, self.F = self.m.shard_plan(self.G)
        self.ctxs, self.wks, self.comms, self.bufs = [], [], [], []
        tables = tables if tables is not None else self.data["tables"]
        try:
            for g in range(self.G):
                c = fr.Context(self.m, device=device, shard_rank=g, n_shards=self.G)
                self.ctxs.append(c)
                for t in held_tables(self.m, self.offs[g], self.lens[g]):   # (a shard of the dense block alone gets none)
                    c.upload_table(t, tables[t])
                for l in range(4):
                    c.set_weights(l, self.data["ws"][l].ravel())
                if prec != "f32":
                    c.set_fc_precision(precision(fr, prec))
                if r.get("width"):
                    c.set_chain_width(r["width"])
                self.wks.append(fr.Worker(c, self.B))
            if comms:
                self.comms = fr.Comm.init_all(self.ctxs)
        except Exception:
            self.close()
            raise

    def close(self):
        for b in self.bufs:
            b.free()
        for w in self.wks:
            w.close()
        for cm in self.comms:
            cm.close()
        for c in self.ctxs:
            c.close()
        self.bufs, self.wks, self.comms, self.ctxs = [], [], [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def on_device(self, arr):
        """One buffer for every rank: the shard contexts share the device (CPU back-end: the host)."""
        b = self.fr.DeviceBuffer.from_numpy(self.ctxs[0], arr)
        self.bufs.append(b)
        return b

    def release(self, b):
        self.bufs.remove(b)
        b.free()

    def ranges(self):
        return [(lo, hi - lo) for lo, hi in (item_range(g, self.G, self.B) for g in range(self.G))]

    def set_act_exponents(self, ae):
        for c in self.ctxs:
            c.set_fp8_act_exponents(ae)

    def fc(self, g, d_gathered, b_total, item0, n, want, what, transport=None):
        """fc_from_slices[_lp] on rank g into a NaN-filled buffer one ldm long: the n scores bit-exact, nothing written past n."""
        fr = self.fr
        ldm = (n + 31) // 32 * 32
        d_s = fr.DeviceBuffer(self.ctxs[g], ldm * 4)
        try:
            d_s.upload(np.full(ldm, np.nan, np.float32))
            if transport is None:
                self.wks[g].fc_from_slices(b_total, item0, n, d_gathered, d_s)
            else:
                self.wks[g].fc_from_slices_lp(b_total, item0, n, d_gathered, transport, d_s)
            self.wks[g].sync()
            got = d_s.download(np.float32, ldm)
        finally:
            d_s.free()
        same(got[:n], want, "%s, rank %d, items [%d, +%d)" % (what, g, item0, n))
        assert np.isnan(got[n:]).all(), "%s, rank %d wrote past its %d items" % (what, g, n)

    def both_layouts(self, gathered, want, what, transport=None):
        """Every rank with an item: its range from the all-gather layout and from the all-to-all layout; one rank also a range off the split."""
        d_g = self.on_device(gathered)
        for g, (lo, n) in enumerate(self.ranges()):
            if n > 0:
                self.fc(g, d_g, self.B, lo, n, want[lo:lo + n], what + " (all-gather layout)", transport)
        if self.B > 1:
            n = min(self.B - 1, 33)
            self.fc(min(1, self.G - 1), d_g, self.B, 1, n, want[1:1 + n], what + " (all-gather layout, off the split)", transport)
        self.release(d_g)
        for g, (lo, n) in enumerate(self.ranges()):
            if n > 0:
                d_m = self.on_device(np.ascontiguousarray(gathered[:, lo:lo + n]))
                self.fc(g, d_m, n, 0, n, want[lo:lo + n], what + " (all-to-all layout)", transport)
                self.release(d_m)

    def step(self, b, mode, want, what):
        """fr_worker_submit_sharded of the first b items on every rank (one thread submits, then the syncs): every rank's b scores."""
        for cm in self.comms:
            cm.set_exchange(mode)
        for w in self.wks:
            w.idx[:b] = self.idx[:b]
            if w.dense is not None:
                w.dense[:b] = self.dense[:b]
            w.score[:] = np.nan
        for g in range(self.G):
            self.wks[g].submit_sharded(self.comms[g], b)
        for g in reversed(range(self.G)):
            self.wks[g].sync()
        for g in range(self.G):
            same(self.wks[g].score[:b], want[:b], "%s, %s step of %d items, rank %d" % (what, mode, b, g))

    def collective(self, fn):
        """fn(rank) on one thread per rank (the synchronous collectives)."""
        errs = [None] * self.G

        def run(g):
            try:
                fn(g)
            except Exception as ex:   # noqa: BLE001
                errs[g] = ex
        ts = [threading.Thread(target=run, args=(g,)) for g in range(self.G)]
        for t in ts:
            t.start()
        for t in ts:
            t.join(120)
        assert not any(t.is_alive() for t in ts)
        assert errs == [None] * self.G, errs


# ---- the checks -----------------------------------------------------------------------------------------------------------------------------
def check_slices(job, ae=None):
    """gather_records on every rank == the host record's slice; in bf16 / fp8 also gather_slices(transport) == the wire form of that slice.
    -> (gathered fp32 [G][B][F], gathered transport form or None), NaN patterns past every slice's length."""
    fr, B, F = job.fr, job.B, job.F
    g32 = np.empty((job.G, B, F), np.float32)
    for g, wk in enumerate(job.wks):
        sl = wk.gather_records(job.idx, job.dense).reshape(B, F)
        o, ln = job.offs[g], job.lens[g]
        assert np.array_equal(sl[:, :ln], job.rec[:, o:o + ln].view(np.uint32)), "fp32 slice of rank %d" % g
        g32[g] = sl.view(np.float32)
    pad_nan(g32, job.lens)
    if job.prec == "f32":
        return g32, None
    P = precision(fr, job.prec)
    dt = np.uint16 if job.prec == "bf16" else np.uint8
    glp = np.empty((job.G, B, F), dt)
    d_i = job.on_device(job.idx)
    d_d = job.on_device(job.dense) if job.dense is not None else None
    d_sl = job.on_device(np.zeros(B * F, dt))
    for g, wk in enumerate(job.wks):
        wk.gather_slices(B, d_i, d_d, d_sl, P)
        wk.sync()
        sl = d_sl.download(dt, B * F).reshape(B, F)
        o, ln = job.offs[g], job.lens[g]
        assert np.array_equal(sl[:, :ln], transported(job.prec, job.rec[:, o:o + ln], ae[0] if ae else 0)), "%s slice of rank %d" % (job.prec, g)
        glp[g] = sl
    return g32, pad_nan(glp, job.lens)


def check_row(fr, device, r, prec):
    """Slices, fp8 calibration on the slices, fc_from_slices[_lp] in both layouts, and the whole step in both exchange modes at B, min(B, G - 1), B."""
    want, ae, we = expect(fr, r, prec)
    heavy = r.get("heavy", False)
    with Job(fr, device, r, prec, comms=r["G"] <= MAX_RANKS) as job:
        if prec == "fp8":   # exponents from the fp32 slices, on one rank; every rank then takes them
            g32 = host_gathered(job.rec, job.offs, job.lens, job.F)
            d_g = job.on_device(g32)
            job.wks[0].calibrate_fp8_slices(job.B, 0, job.B, d_g)
            job.release(d_g)
            assert job.ctxs[0].fp8_exponents() == (ae, we), (job.ctxs[0].fp8_exponents(), ae, we)
            job.set_act_exponents(ae)
        g32, glp = check_slices(job, ae)
        job.both_layouts(g32, want, "fp32 slices")
        if glp is not None and not heavy:
            job.both_layouts(glp, want, "%s slices" % prec, precision(fr, prec))
            other = fr.FC_FP8 if prec == "bf16" else fr.FC_BF16
            d_g, d_s = job.on_device(glp), job.on_device(np.zeros(32, np.float32))
            try:
                job.wks[0].fc_from_slices_lp(job.B, 0, 1, d_g, other, d_s)
                raise AssertionError("a transport that is not the context's precision was accepted")
            except fr.FleetRecError as ex:
                assert ex.status == fr.FR_ERR_STATE, ex
        if heavy and device != CPU:
            names = []
            n = job.ranges()[0][1]
            for l in range(4):
                job.wks[0].fc_layer_only(n, l)
                names.append(job.wks[0].last_kernel())
                job.wks[0].sync()
            assert names == r["layers"][prec], names
        if not job.comms:
            try:
                fr.Comm.init_all(job.ctxs)
                raise AssertionError("fr_comm_init_all took %d ranks" % job.G)
            except fr.FleetRecError as ex:
                assert ex.status == fr.FR_ERR_INVALID, ex
            return
        if prec == "fp8":   # the collective calibration gives every rank the same exponents again
            job.set_act_exponents([0, 0, 0, 0])
            job.collective(lambda g: job.wks[g].calibrate_fp8_sharded(job.comms[g], job.idx, job.dense))
            for c in job.ctxs:
                assert c.fp8_exponents() == (ae, we), (c.fp8_exponents(), ae, we)
        if heavy:
            job.step(job.B, "allgather", want, prec)
            return
        for mode in ("allgather", "alltoall"):
            for b in (job.B, min(job.B, job.G - 1), job.B):
                job.step(b, mode, want, prec)


def check_dense_only_shard_loads_by_upload(fr, device):
    """Row g's shard 12 is the dense block alone: no table is resident, every upload to it is refused, and it answers gather_records at once."""
    r = row("g")
    m, data, idx, dense, rec = batch(fr, r)
    offs, lens, F = m.shard_plan(r["G"])
    g, ln = r["plan"]["dense_only"]
    assert held_tables(m, offs[g], lens[g]) == [] and lens[g] == ln
    c = fr.Context(m, device=device, shard_rank=g, n_shards=r["G"])
    wk = fr.Worker(c, r["B"])
    try:
        for t in (0, m.n_tables - 1):
            try:
                c.upload_table(t, data["tables"][t])
                raise AssertionError("a shard without tables took an upload of table %d" % t)
            except fr.FleetRecError as ex:
                assert ex.status == fr.FR_ERR_STATE, ex
        sl = wk.gather_records(idx, dense).reshape(r["B"], F)
        assert np.array_equal(sl[:, :ln], rec[:, offs[g]:offs[g] + ln].view(np.uint32))
    finally:
        wk.close()
        c.close()


def check_nan_table_value(fr, device, prec):
    """Row c with a NaN in one table row of a middle shard, hit by exactly two items: those two scores are NaN, every other score is bit-exact
    (fc_from_slices on every rank, then one step).  The fp8 exponents are those of the clean batch."""
    r = row("c")
    m, data, idx, dense, _ = batch(fr, r)
    _, ae, we = expect(fr, r, prec)   # (premise and witnesses of the clean batch; fp8: its exponents)
    offs, lens, _ = m.shard_plan(r["G"])
    g_mid = r["G"] // 2
    t = held_tables(m, offs[g_mid], lens[g_mid])[1]
    col = next(s.rec_offset for s in m.segments() if s.kind != SEG_DENSE and s.src == t) + 1
    hit = [5, r["B"] - 3]
    bad_row = int(idx[hit[0], t])
    idx = idx.copy()
    idx[idx[:, t] == bad_row, t] = (bad_row + 1) % data["tables"][t].shape[0]
    idx[hit, t] = bad_row
    tables = list(data["tables"])
    tables[t] = tables[t].copy()
    tables[t][bad_row, 1] = np.nan
    rec_n = E.records(m, dict(data, tables=tables), idx, dense)
    assert np.flatnonzero(np.isnan(rec_n).any(axis=1)).tolist() == hit and np.isnan(rec_n[hit, col]).all()
    clean = np.where(np.isnan(rec_n), np.float32(0), rec_n)
    E.premise(prec, clean, data["ws"], ae, we)
    want_n = E.expected(prec, clean, data["ws"], ae, we)
    want_n[hit] = np.nan
    with Job(fr, device, r, prec, tables=tables, comms=True) as job:
        job.idx, job.rec = idx, rec_n
        if prec == "fp8":
            job.set_act_exponents(ae)
        g32 = np.empty((job.G, job.B, job.F), np.float32)
        for g, wk in enumerate(job.wks):
            g32[g] = wk.gather_records(idx, dense).reshape(job.B, job.F).view(np.float32)
            o, ln = offs[g], lens[g]
            assert np.array_equal(g32[g, :, :ln].view(np.uint32), rec_n[:, o:o + ln].view(np.uint32))
        d_g = job.on_device(pad_nan(g32, lens))
        for g, (lo, n) in enumerate(job.ranges()):
            job.fc(g, d_g, job.B, lo, n, want_n[lo:lo + n], "a NaN table value")
        job.step(job.B, "allgather", want_n, "a NaN table value")
        for g in range(job.G):
            assert np.flatnonzero(np.isnan(job.wks[g].score[:job.B])).tolist() == hit


def check_fp8_calibration_ignores_stale_padding(fr, device):
    """The sharded twin of test_exact_fp8_calibration_ignores_stale_padding: calibrate on 64 large-activation items of the pool, then on a window
    (item0 = 71, n = 33: the same ldm of 64, item0 off the 16-item tile) of small ones -- the exponents are the window's."""
    r = row("c")
    m, data, pool = model_data(fr, r["model"])
    ws = data["ws"]
    acts, _ = E.fp32_acts(pool, ws)
    order = np.argsort(np.abs(acts[1]).max(axis=1))
    big, small = order[-64:], order[:33]
    sel = np.concatenate([big, big[:7], small])
    e_big, e_small = E.act_exponents(pool[big], ws), E.act_exponents(pool[small], ws)
    assert e_big != e_small   # (else the check below proves nothing)
    offs, lens, F = m.shard_plan(r["G"])
    c = fr.Context(m, device=device, shard_rank=0, n_shards=r["G"])
    wk = None
    try:
        for l in range(4):
            c.set_weights(l, ws[l].ravel())
        c.set_fc_precision(fr.FC_FP8)
        wk = fr.Worker(c, 64)
        d_g = fr.DeviceBuffer.from_numpy(c, host_gathered(pool[sel], offs, lens, F))
        wk.calibrate_fp8_slices(len(sel), 0, 64, d_g)
        assert c.fp8_exponents() == (e_big, E.w_exponents(ws)), (c.fp8_exponents(), e_big)
        wk.calibrate_fp8_slices(len(sel), 71, 33, d_g)
        assert c.fp8_exponents()[0] == e_small, (c.fp8_exponents()[0], e_small)
        d_s = fr.DeviceBuffer(c, 64 * 4)
        d_s.upload(np.full(64, np.nan, np.float32))
        wk.fc_from_slices(len(sel), 71, 33, d_g, d_s)
        wk.sync()
        got = d_s.download(np.float32, 64)
        E.premise("fp8", pool[small], ws, e_small, E.w_exponents(ws))
        same(got[:33], E.expected("fp8", pool[small], ws, e_small, E.w_exponents(ws)), "fc_from_slices after recalibration")
        assert np.isnan(got[33:]).all()
        d_g.free()
        d_s.free()
    finally:
        if wk:
            wk.close()
        c.close()


# ---- simulated bugs of the slice re-pack, applied on the host (tests/test_cpu_exact_sharded.py) ------------------------------------------------
def assemble(gathered, offs, lens, K, item0, n):
    """Records [n][K] of items [item0, item0 + n) from the all-gathered slices [G][B][F]: what the slice transposes build."""
    return assemble_records(np.nan_to_num(gathered[:, item0:item0 + n], nan=0.0), offs, lens, K)


def mutant_records(name, gathered, offs, lens, K, item0, n):
    """The records a slice re-pack with the named bug would build for items [item0, item0 + n); None where the plan has no place for the bug."""
    G = len(offs)
    rec = assemble(gathered, offs, lens, K, item0, n)
    if name == "first_word":      # the first word of a shard's slice taken from the neighbouring shard (same word of its slice)
        g = G // 2 if G > 1 else None
        if g is None or g < 1:
            return None
        rec[:, offs[g]:offs[g] + 4] = np.nan_to_num(gathered[g - 1, item0:item0 + n, 0:4])
        return rec
    if name == "last_word":       # the last word of a slice whose length is no multiple of 16 words comes out as zeros
        g = next((g for g in range(G) if lens[g] // 4 % 16), None)
        if g is None:
            return None
        rec[:, offs[g] + lens[g] - 4:offs[g] + lens[g]] = 0
        return rec
    if name == "item0":           # the item window starts one item late
        if item0 + 1 + n > gathered.shape[1]:
            return None
        return assemble(gathered, offs, lens, K, item0 + 1, n)
    if name == "bf16_pair":       # a shard boundary on an odd record word: the two words of that operand pair land in each other's half
        g = next((g for g in range(1, G) if offs[g] // 4 % 2), None)
        if g is None:
            return None
        w = offs[g] // 4          # odd: words w - 1 (end of shard g - 1) and w (start of shard g) share a bf16 element of 8 k
        rec[:, 4 * (w - 1):4 * w], rec[:, 4 * w:4 * (w + 1)] = rec[:, 4 * w:4 * (w + 1)].copy(), rec[:, 4 * (w - 1):4 * w].copy()
        return rec
    if name == "shard_order":     # shards 63 and 64 (the last of one launch's slice table, the first of the next) exchanged
        if G < 65:
            return None
        g2 = gathered.copy()
        g2[[63, 64]] = g2[[64, 63]]
        return assemble(g2, offs, lens, K, item0, n)
    raise KeyError(name)


def fp8_pad_mutant_scores(rec, ws, ae, we):
    """The fp8 chain restated with FC1's K padded to a multiple of 64 as the operand image has it, the pad k of the activations holding a stale
    e4m3 NaN byte in place of zero (the weights' pad rows are zero): the scores such an image gives (a NaN in FC1's sums stays a NaN to the end:
    the chain's clamps are compares, its conversions keep it)."""
    dec = e4m3_decode_table()
    K = rec.shape[1]
    KP = (K + 63) // 64 * 64
    x = np.full((rec.shape[0], KP), dec[0x7F])
    x[:, :K] = dec[e4m3_encode(np.asarray(rec, np.float32) * np.float32(2.0 ** ae[0]))]
    W = np.zeros((KP, ws[0].shape[1]))
    W[:K] = dec[e4m3_encode(ws[0] * np.float32(2.0 ** we[0]))]
    with np.errstate(invalid="ignore"):
        r1 = x @ W
    return np.where(np.isnan(r1).any(axis=1), np.float32(np.nan), E.expected("fp8", rec, ws, ae, we))

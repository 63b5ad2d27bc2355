// Internal declarations shared by the host-side C-ABI (fr_api.cpp, fr_registry.cpp) and the
// gfx950 kernels (fr_fill / fr_gather / fr_pipeline / fr_gemm / fr_fused .hip).  Not installed; the public surface is include/fleetrec.h (+ fleetrec_serving.h, fleetrec_diag.h).
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <cstdint>
#include <string>
#include <vector>

#include "fleetrec.h"
#include "fleetrec_diag.h"
#include "fleetrec_serving.h"
#include "fr_keys.h"
#include "fr_mem.h"

// ---- error plumbing ---------------------------------------------------------------------------
void fr_set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));

#define FR_FAIL(code, ...)         \
    do {                           \
        fr_set_error(__VA_ARGS__); \
        return (code);             \
    } while (0)

#define FR_HIP(call)                                                                                 \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) {                                                                      \
            fr_set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? FR_ERR_OOM : FR_ERR_HIP;                            \
        }                                                                                            \
    } while (0)

#define FR_TRY(expr)               \
    do {                           \
        const int rc_ = (expr);    \
        if (rc_) return rc_;       \
    } while (0)

// ---- experiment knobs ---------------------------------------------------------------------------
// The product library reads NO environment variable: FR_KNOB folds to its default and the variable's name is not even in the
// binary.  `make exp` builds libfleetrec_exp.so with -DFR_EXPERIMENTS, where FR_KNOB("X", d) reads the environment variable FR_X
// (FR_KNOB: at every call -- in-process sweeps; FR_KNOB_ONCE: once per process); A/B runs load that build through FR_LIB.
#ifdef FR_EXPERIMENTS
int fr_knob_env(const char *name, int dflt);
#define FR_KNOB(name, dflt) fr_knob_env("FR_" name, (dflt))
#define FR_KNOB_ONCE(name, dflt) ([]() -> int { static const int v_ = fr_knob_env("FR_" name, (dflt)); return v_; }())
#else
#define FR_KNOB(name, dflt) (dflt)
#define FR_KNOB_ONCE(name, dflt) (dflt)
#endif

// ---- which kernel ran ---------------------------------------------------------------------------
// Every launcher names the kernel it just enqueued (instantiation included, as rocprofv3 prints it) in a thread-local note; the entry
// points of the C-ABI copy the note of their dominant launch into the worker (fr_worker_last_kernel), so that bench.py's roofline
// objects name the kernel that actually ran instead of the one the author expected.
void fr_note_kernel(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *fr_noted_kernel();

// ---- device-side descriptors --------------------------------------------------------------------
// One per 16-byte word of the per-item record (the unit the reference's packers move:
// `typedef ap_uint<128> axi_t`, constants.hpp:4).  32 bytes = two dwordx4 loads, read once per thread.
struct FrWordDesc {
    uint64_t src;        // TABLE/COPY: device address of (table base + 16*word_in_row); DENSE: byte offset in the item's dense row
    uint32_t stride;     // bytes between consecutive rows of the source (dim*4; DENSE: dense_len*4)
    uint32_t idx_col;    // column of the item's index row feeding this word (0 in PER_ITEM mode); bit 31 set = DENSE
    uint32_t rows;       // row count for the range check (DENSE: unused)
    uint32_t dst_off;    // word offset inside the item's destination row
    uint32_t dst_stride; // words per item of the destination block (SEMANTIC: K/4; BLOCKED: source_len/4)
    uint32_t dst_blk;    // BLOCKED: words-per-item of all preceding source blocks (x batch at run time); SEMANTIC: 0
};
static_assert(sizeof(FrWordDesc) == 32, "FrWordDesc must be 32 bytes");
#define FR_DESC_DENSE 0x80000000u

// How gather_pack_xcd_kernel deals the record words to the 8 XCD groups: group g owns words [start[g], start[g + 1]).  The cuts
// sit on SOURCE-ROW boundaries (a table row, or a whole bank row of a bank-interleaved context): a row cut in two would be fetched
// by two XCDs -- the same 128-byte line through two L2s.  max_words = the widest group (the kernel's block size).
struct FrGatherGroups {
    int start[9];
    int max_words;
};

// Pooled (multi-hot) gather, gather_pooled_kernel: one per FrWordDesc, in the same order.  The word's bag of the item's pooled index
// row idx[P] is idx[first .. first + hots); a DENSE word has hots == 1 (its one "slot" is the item itself).  FrWordDesc::idx_col is not
// read by the pooled kernel but for its DENSE bit.  The word's pooling mode rides in the spare high bit of `hots` (its maximum is 64):
// FR_POOL_DESC_MEAN set = the fold is divided by the bag's count of non-empty slots (never set on a DENSE word).
constexpr uint32_t FR_POOL_DESC_MEAN = 0x80000000u;
struct FrPoolDesc {
    uint32_t first;   // first pooled index column of the word's bag
    uint32_t hots;    // slots of the bag (1 .. FR_POOL_MAX_HOTS) | FR_POOL_DESC_MEAN
};
static_assert(sizeof(FrPoolDesc) == 8, "FrPoolDesc must be 8 bytes");
// Where gather_pooled_kernel stores its folded words, uniform over the launch: the kernel's view of FrPooledOut, packed by frk_gather_pooled.  ldm == 0: the item's fp32 record (16 bytes at the word's place in the
// model's layout).  form 1 / 2 / 3: straight into the chain's feature-major stage-1 operand of `ldm` items, in the chain's operand type -- fp32
// Xq[K/4][ldm] (16 bytes, a bit copy), bf16 Xh[K/8][ldm] (8 bytes, RNE), e4m3 Xf[KE][ldm] (4 bytes, x scale, saturated); 16-byte elements, element
// (w >> (form - 1), b) holds word w of item b.  The launch writes the whole region a stage reads: pad items [batch, ldm) and the pad words
// of the k-rows past the record are zeros.
constexpr int FR_POOL_NO_OPERAND_ARM = 1;   // frk_gather_pooled into an OPERAND: not an error, not a launch
struct FrPoolDest {
    unsigned ldm;   // 0: records; FR_PD_ROWS: 16-byte words per item of the item-major destination
    int code;       // the FR_PD_* fields below, packed by frk_gather_pooled: one scalar register in the kernel instead of four
};
// fields of FrPoolDest::code, shared by the launcher and the kernel
constexpr unsigned FR_PD_FORM_MASK = 3u;                            // bits 0-1: the form (1 fp32, 2 bf16, 3 e4m3)
constexpr unsigned FR_PD_PAD_SHIFT = 2, FR_PD_PAD_MASK = 63u;       // bits 2-7: pad words behind the record in the operand's k-rows
constexpr unsigned FR_PD_FOLD_SHIFT = 8, FR_PD_FOLD_MASK = 7u;      // bits 8-10: the fold, FR_PD_FOLD_*
// bit 11: the ITEM-MAJOR destination of forms 2 / 3 -- a shard's low-precision slice [batch][ldm words] (fr_worker_gather_slices_pooled): `ldm` is then
// the destination's 16-byte-word count per item (slice_padded / 4), word w of item b goes to b * ldm * (16 >> sh) + w * (16 >> sh) bytes, nothing is
// zero-filled and no item past the batch is written
constexpr unsigned FR_PD_ROWS = 1u << 11;
constexpr unsigned FR_PD_EX_SHIFT = 16;                             // bits 16-31, signed: form 3's X exponent e_x (scale 2^e_x; an arithmetic shift recovers it)
constexpr unsigned FR_PD_FOLD_SUM = 0u, FR_PD_FOLD_MEAN = 1u, FR_PD_FOLD_WEIGHTED = 2u, FR_PD_FOLD_CSR = 3u, FR_PD_FOLD_CSR_WEIGHTED = 4u;

// A pooled batch as the caller handed it in, from the C-ABI's entry points down to both gather back-ends (device pointers; host memory on the CPU
// back-end).  Padded form: idx = int32 [batch][P] (-1: an empty slot), weights = NULL or float [batch][P].  Offsets (CSR) form (offsets != NULL):
// offsets = int32 [batch * index columns + 1], idx / weights = the nnz flat entries.  weights != NULL selects the weighted fold.
struct FrPooledBatch {   // (brace-initialised in this order by the entry points)
    int batch = 0;
    const int32_t *idx = nullptr;
    const float *weights = nullptr, *dense = nullptr;
    const int32_t *offsets = nullptr;
    int64_t nnz = 0;
    bool need_weights = false;   // the call came through a *_weighted entry point: weights must be there
};
// Where the folded words go.  RECORDS: fp32 records in the model's layout (a shard: its fp32 slice).  OPERAND: the chain's feature-major stage-1 operand of
// `ldm` items in `precision` (FrPoolDest forms 1 / 2 / 3), written whole.  LP_SLICE: a shard's item-major slice in the transport `precision` (bf16 / e4m3).
struct FrPooledOut {
    enum Kind { RECORDS, OPERAND, LP_SLICE };
    void *ptr = nullptr;
    Kind kind = RECORDS;
    int precision = FR_FC_FP32, ldm = 0;
};
// What the context and the worker add to a launch (fr_ctx's fields of the same names; host arrays on the CPU back-end): filled by pooled_plan
// (fr_api.cpp), the one place that picks the padded or the offsets form's descriptors (`pool`) and clears `wide` for the latter
struct FrPooledPlan {
    const FrWordDesc *words = nullptr;
    const FrPoolDesc *pool = nullptr;
    const FrGatherGroups *groups = nullptr;   // GPU only
    int n_words = 0, out_words = 0;           // record words gathered / 16-byte words per item of the destination
    int pool_cols = 0, max_hots = 0, n_icols = 0, e_x = 0;
    bool wide = false, any_mean = false;
    int *err_flag = nullptr;
};

// One wave-instruction of the item-tile gather (gather_tile_kernel, fr_gather.hip): 64 / n_words items x n_words consecutive
// 16-byte words of ONE source row each (n_words = 1, 2, 4, 8 or 16: a whole table row, or a power-of-two piece of one).  A record
// segment of w words appears as w passes (item0 = 0, 64/w, 2*64/w, ...) so that the passes of a 64-item tile cover every item.
struct FrPassDesc {
    uint64_t src;        // TABLE/COPY: device address of the piece inside row 0; DENSE: byte offset inside the item's dense row
    uint32_t stride;     // bytes between rows of the source
    uint32_t idx_col;    // index column (bit 31: DENSE)
    uint32_t rows;       // range check (DENSE: unused)
    uint16_t tile_word;  // first word of the piece inside the chunk's LDS tile row
    uint8_t log2_words;  // log2(n_words)
    uint8_t item0;       // first item of the tile this pass serves
    uint32_t pad_;
};
static_assert(sizeof(FrPassDesc) == 32, "FrPassDesc must be 32 bytes");
constexpr int FR_TILE_ITEMS = 64, FR_TILE_WORDS = 64;  // gather_tile_kernel: items per workgroup, record words per chunk
struct FrChunkDesc {
    int pass_begin, pass_end;  // passes of the chunk inside ctx->d_passes
    int word0, n_words;        // the chunk's word range inside the item's destination row
};

// ---- per-layer epilogue (fr_ctx_set_epilogue, fleetrec_serving.h) --------------------------------------
// What a kernel that finishes a layer applies to the layer's fp32 sums before it stores them: v = sum + bias[n] (ONE fp32 add after the whole
// K sum), then ReLU, then the chain's own rounding.  Both members are wave-uniform kernel arguments; {NULL, 0} is the chain as it always was,
// bit for bit (no add at all: -0 stays -0).  The output layer's entry carries b_3 in bias[0] and never an activation.
struct FrEpi {
    const float *bias;   // [N] fp32 (device memory; host memory on the CPU back-end) or NULL
    int relu;            // 1: FR_ACT_RELU
    int pad_;
};

// ---- pipelined FC chain: launch arguments (see fr_pipeline.hip) ------------------------------------
constexpr int FR_N_STAGES = 5;  // gather | FC1 | FC2 | FC3 | out

struct FrStageArgs {
    int block_begin;  // first workgroup of this stage inside the launch; == next stage's begin when inactive
    int batch;        // real items
    int ldm;          // padded items (multiple of 32) = leading dimension of every activation matrix of this batch
    int K, N;         // FC stages: reduction length / outputs; out stage: K = H3
    int nsplit;       // FC stages: workgroups along K per output tile (partials written to out + p*part_stride);
                      // K % (8 * nsplit) == 0 is required (groups of 8 k)
    int nparts_in;    // FC/out stages: partial inputs to add while loading (1 or 2)
    int variant;      // gather stage: LDS-transposing forms for large batches, 1 = gather_tr_body, 2 = gather_tr_stream_body
    int part_stride;  // floats between the partial OUTPUT buffers
    int in_part_stride;  // floats between the partial INPUT buffers
    int e_w, e_in, e_out;  // fp8 chain: power-of-two quantisation exponents of the weights, the input and the output activations
    const float *in;  // activations in (feature-major)
    float *out;       // activations out / scores
    const float *w;   // weights Wt[K][N] (FC) or w[H] (out)
};

struct FrPipeCore {   // what the kernels of libfleetrec.so take: the parent's kernel arguments, byte for byte
    FrStageArgs st[FR_N_STAGES];
    int n_blocks;
    // gather stage
    const struct FrWordDesc *words;
    int src_lp;   // 1: `words` address the operand-type bank image (rows already bf16 / e4m3: 8 / 4 bytes per record word); dense words stay fp32
    int n_words;
    int idx_stride;
    const int32_t *idx;
    const float *dense;
    int *err_flag;
    // diagnostic build aid (NULL in normal operation): per workgroup {s_memrealtime at entry, at exit, stage, hw id}
    unsigned long long *stamps;
};
struct FrPipeArgs : FrPipeCore {
    // Epilogues per stage (pipeline_step, fr_api.cpp).  Only the epilogue forms of the kernels (libfleetrec_epi.so) take this part as kernel arguments;
    // has_epi == 0 sends the launch to the kernels of libfleetrec.so, which take the FrPipeCore slice.  epi[s]: stage s's own layer, applied where the stage
    // stores WHOLE sums (nsplit == 1; the out stage: bias[0] added to the score) -- left {NULL, 0} on a split stage, whose partials are stored raw.
    // epi_in[s]: the PRODUCING layer's, set only where stage s reads two partials (nparts_in == 2): it applies it to their sum while loading.
    FrEpi epi[FR_N_STAGES], epi_in[FR_N_STAGES];
    int has_epi;
};

// ---- fused item-tile kernel: launch arguments (see fr_fused.hip) -------------------------------------
constexpr int FR_FUSED_MAX_BATCHES = 64;   // kernel-argument array size (64 x 32 B): what one launch of the kernarg-fed kernels carries
constexpr int FR_FUSED_MAX_QUEUE = 256;    // batches a worker queues / the persistent bf16 kernel carries per launch (its list lives in device memory)
constexpr int FR_BLIST_RING = 4;           // staging blocks of that list per worker
constexpr int FR_FUSED_DEFAULT_BATCHES = 64;
constexpr int FR_FUSED_MIN_GROUP = 12;       // fr_worker_push_device: smaller launch groups ride the stage pipeline (one launch per push)
constexpr int FR_HOST_BLOCKS = 4;  // 64 batches of 256 = one 64-item workgroup per CU (fr_fused_tile_m2_kernel)
struct FrFusedBatch {
    const int32_t *idx;
    const float *dense;
    float *scores;
    int batch;
    int pad_;
};
struct FrFusedArgs {
    FrFusedBatch b[FR_FUSED_MAX_BATCHES];
    int n_batches;
    int tiles_per_batch;  // max over the batches of ceil(batch / 32)
    const struct FrWordDesc *words;
    int src_lp;   // 1: `words` address the operand-type bank image (rows already bf16 / e4m3: 8 / 4 bytes per record word); dense words stay fp32
    int n_words;
    int idx_stride;
    int *err_flag;
    const FrFusedBatch *blist;      // fr_fused_tile_hs_kernel: the launch's batches in device memory (up to FR_FUSED_MAX_QUEUE; b[] is unused then)
    const float4 *w1q, *w2q, *w3q;  // q4-packed weights
    const float *wout;
    int K, H1, H2, H3;
    int e_w[3], e_act[4];        // fp8 kernel only: quantisation exponents (weights W1..W3; activations X, R1, R2, R3)
    unsigned long long *stamps;  // diagnostics only (NULL normally): 16 s_memrealtime stamps per workgroup
    // per-layer epilogues (FC1, FC2, FC3, output).  All {NULL, 0} without fr_ctx_set_epilogue: the launchers run fr_fused_tile_*_kernel.  With one, EVERY
    // bias pointer is set (a layer without a bias points at -0.0f values) and the launchers run the branch-free fr_epi_tile_*_kernel forms.
    // fr_fused_tile_hs_kernel does not read them: a context with an epilogue never launches it (fr_fused_flush, fr_api.cpp)
    FrEpi epi[4];
};

// ---- epilogue forms of the FC-chain kernels (libfleetrec_epi.so, the fourth companion code object) ------------------------------------------------
// fr_fused.hip, fr_pipeline.hip and fr_gemm.hip built a second time with -DFR_EPI_FORMS: the same bodies under names of their own (fr_epi_tile_*_kernel,
// fr_epi_pipeline_kernel, fr_epi_gather_out_kernel, fc_epi_*gemm*_kernel), which apply the per-layer epilogues; the kernels of libfleetrec.so carry no
// epilogue code.  Three exported launchers, one per file; each enqueues on `stream` (a hipStream_t), names the kernel in name[0 .. name_len) and
// -> 0 or the hipError_t value.  (The FR_* experiment knobs do not reach them: the companion is a product build, also beside libfleetrec_exp.so.)
// fr_epi_fused_launch: the epilogue form of the fused launcher `kind`.
constexpr int FR_EPI_KIND_F32 = 0, FR_EPI_KIND_F32_M2 = 1, FR_EPI_KIND_BF16 = 2, FR_EPI_KIND_FP8 = 3;
extern "C" int fr_epi_fused_launch(const FrFusedArgs *args, int kind, void *stream, char *name, size_t name_len);
// fr_epi_pipeline_launch: frk_pipeline_launch's arguments.  fr_epi_gemm_launch:
struct FrEpiGemmCall {   // the arguments of frk_fc_lp_gemm (tail == 0) or frk_fc_tail (tail == 1: Yp = wout, scores / batch set, epi = FC3's)
    int tail, precision;
    const void *Wp, *Xp;
    void *Yp;
    float *scores;
    int K, N, ldm, batch, e_w, e_in, e_out, width, minor;
    FrEpi epi, epi_out;
};
extern "C" int fr_epi_pipeline_launch(const FrPipeArgs *args, int single_stage, int precision, void *stream, char *name, size_t name_len);
extern "C" int fr_epi_gemm_launch(const FrEpiGemmCall *call, void *stream, char *name, size_t name_len);

// ---- segmented top-K ranking (fr_rank.hip -> libfleetrec_rank.so, the companion code object; fr_cpu.cpp has the twin) ------------------------
// The rank order of fleetrec_serving.h on a score's 32 bits: a larger key ranks first; every NaN has key 0, behind -inf (0x007fffff).
static inline __host__ __device__ uint32_t fr_rank_key(uint32_t u) { return (u & 0x7fffffffu) > 0x7f800000u ? 0u : ((u & 0x80000000u) ? ~u : (u | 0x80000000u)); }
constexpr int FR_RANK_PART = 16384;      // scores one workgroup streams: a longer segment is cut into units of this many
constexpr int FR_RANK_FAN = 16;          // candidate lists one merge workgroup folds (16 x FR_TOPK_MAX_K composites = one LDS tile)
constexpr size_t FR_RANK_HDR_BYTES = 16; // the scratch's head: [0] units reserved so far
struct FrRankArgs {
    const float *scores;
    const int32_t *off;      // [n_seg + 1], or NULL: one segment [0, n)
    int n, n_seg, k;
    int u_cap;               // unit records / candidate lists the scratch holds (0 without scratch)
    int32_t *top_idx;        // [n_seg][k]
    float *top_scores;       // [n_seg][k] or NULL
    int *err_flag;
    // worker-owned scratch of segments longer than FR_RANK_PART (all NULL when n <= FR_RANK_PART: no segment can be)
    int *hdr;
    int4 *unitmap;                // [u_cap] {segment, part, parts of the segment, 0}; x < 0: no unit
    unsigned long long *cand;     // [u_cap][k] composites, descending, 0-padded
};
// units a call over n scores can need when no two segments overlap (they can beside malformed ones; the surplus is ranked by one workgroup each)
static inline int fr_rank_units(int n) { return n > FR_RANK_PART ? 2 * ((n + FR_RANK_PART - 1) / FR_RANK_PART) + 2 : 0; }
// Enqueues the ranking on `stream` (a hipStream_t); wave_form: one wave per segment instead of a 256-thread workgroup.  -> 0 or the hipError_t value.
extern "C" int fr_rank_launch(const FrRankArgs *args, int wave_form, void *stream);

// ---- request-form batches (fr_request.hip -> libfleetrec_request.so, the second companion code object; fr_cpu.cpp has the twin) ----------------
// Row i of `out` ([batch][W] 32-bit words) is put together word by word: desc[w] >= 0 names word desc[w] of candidate row i ([batch][Rc]),
// desc[w] < 0 names word ~desc[w] of the request row ([n_req][Rs]) of the request that owns item i -- the last r with off[r] <= i, clamped into
// [0, n_req); off == NULL: n_req equal requests of batch / n_req items.  Words are bit copies.
constexpr int FR_REQ_TILE_MAX = 64;      // items one workgroup expands at most (their owners sit in LDS)
constexpr int FR_REQ_TILE_WORDS = 8192;  // output words a workgroup aims at: the tile is FR_REQ_TILE_WORDS / W items, 1 .. FR_REQ_TILE_MAX
struct FrRequestArgs {
    const int32_t *off;      // [n_req + 1] or NULL
    const uint32_t *req;     // [n_req][Rs]
    const uint32_t *cand;    // [batch][Rc]; may be NULL when Rc == 0
    uint32_t *out;           // [batch][W]
    const int32_t *desc;     // [W]
    int batch, n_req;
    int W, Rs, Rc;
    int tile;                // items per workgroup, 1 .. FR_REQ_TILE_MAX
    int *err_flag;           // raised when off is malformed (off[0] != 0, a decreasing pair, off[n_req] != batch)
};
static inline int fr_request_tile(int W) {
    const int t = FR_REQ_TILE_WORDS / (W > 0 ? W : 1);
    return t < 1 ? 1 : (t > FR_REQ_TILE_MAX ? FR_REQ_TILE_MAX : t);
}
// Enqueues the one expansion launch on `stream` (a hipStream_t).  -> 0 or the hipError_t value.
extern "C" int fr_request_launch(const FrRequestArgs *args, void *stream);

// ---- keyed lookups (fr_keys.hip -> libfleetrec_keys.so, the third companion code object; fr_cpu.cpp has the twins; fr_keys.h: slot, mix64, probe) ----
constexpr int FR_KEY_PER_THREAD = 4;     // keys a thread of key_resolve_kernel resolves per chunk: their first probes are in flight together
struct FrKeyResolveArgs {
    const int64_t *keys;         // [total], 8-byte aligned
    int32_t *out;                // [total]
    const FrKeyCol *cols;        // [n_cols]
    const uint16_t *wcol;        // [W]: the index column of every word of a row
    unsigned long long *misses;  // the worker's counter of MAPPED lookups that found no key
    uint64_t total;              // n_rows * W
    int W, n_cols;
    int max_blocks;              // workgroups the launch takes at most (they stride over the chunks of 256 x FR_KEY_PER_THREAD words)
};
struct FrKeyPutArgs {
    FrKeyCol col;                // a MAPPED column
    uint32_t *n_keys;            // the column's key count
    uint32_t max_keys;
    int n;
    const int64_t *keys;         // [n]
    const int32_t *rows;         // [n]
    int *err_flag;               // FR_KEYS_ERR_* bits
};
struct FrKeyFillArgs {
    FrKeySlot *slots;
    uint64_t n;
    int32_t miss_row;
};
// Each enqueues its one launch on `stream` (a hipStream_t).  -> 0 or the hipError_t value.
extern "C" int fr_key_resolve_launch(const FrKeyResolveArgs *args, void *stream);
extern "C" int fr_key_put_launch(const FrKeyPutArgs *args, void *stream);
extern "C" int fr_key_fill_launch(const FrKeyFillArgs *args, void *stream);

// ---- the life cycle of a key map (fr_keymaint.hip -> libfleetrec_keymaint.so, the fifth companion code object; fr_cpu.cpp has the twins) ----
constexpr int FR_KEYMAINT_PER_THREAD = 4;   // slots a thread of keymap_walk_kernel loads per trip before its first compare
enum { FR_KEYWALK_COUNT = 0, FR_KEYWALK_EXPORT = 1, FR_KEYWALK_REHASH = 2 };
struct FrKeyEraseArgs {
    FrKeyCol col;                // a MAPPED column
    int n;
    const int64_t *keys;         // [n]
    int *err_flag;               // FR_KEYS_ERR_ERASE_EMPTY
};
struct FrKeyWalkArgs {
    FrKeyCol col;                // the map that is walked
    int sink;                    // FR_KEYWALK_*
    int max_blocks;              // workgroups the launch takes at most (they stride over chunks of 256 x FR_KEYMAINT_PER_THREAD slots)
    unsigned long long *counts;  // COUNT: [0] occupied, [1] live, [2] probe_sum; EXPORT: [0] the pairs reserved; REHASH: [0] the pairs inserted
    int64_t *out_keys;           // EXPORT: [cap]
    int32_t *out_rows;           // EXPORT: [cap]
    uint64_t cap;
    FrKeyCol dst;                // REHASH: the new map (its seed, mask and slots; pre-filled)
};
// Each enqueues its one launch on `stream` (a hipStream_t).  -> 0 or the hipError_t value.
extern "C" int fr_keymap_erase_launch(const FrKeyEraseArgs *args, void *stream);
extern "C" int fr_keymap_walk_launch(const FrKeyWalkArgs *args, void *stream);

// ---- row pools: admitting ids (fr_keyadmit.hip -> libfleetrec_admit.so, the sixth companion code object; fr_cpu.cpp has the twins; fr_keys.h: FrKeyPool) ----
constexpr int FR_KEYADMIT_PER_THREAD = 4;   // slots a thread of keyadmit_mark_kernel loads per trip before its first compare
struct FrKeyAdmitArgs {
    FrKeyCol col;                // a MAPPED column with a pool
    FrKeyPool pool;
    uint32_t *n_keys;            // the column's key count
    uint32_t max_keys;
    int n;
    const int64_t *keys;         // [n]
    int32_t *rows_out;           // [n]
    FrKeySlot *tab;              // the call's own table of tab_mask + 1 >= 2 n slots, pre-filled {-1, FR_KEYS_NO_ROW}: ONE occurrence of every key of the
    uint32_t tab_mask;           //   call admits it, the others take its row from here (keyadmit_settle_kernel); the CPU twin needs none (NULL)
    int *err_flag;               // FR_KEYS_ERR_* bits
};
struct FrKeyReleaseArgs {
    FrKeyCol col;
    FrKeyPool pool;
    int n;
    const int64_t *keys;         // [n]
    int *err_flag;               // FR_KEYS_ERR_ERASE_EMPTY
};
struct FrKeyMarkArgs {
    FrKeyCol col;                // the map that is walked
    FrKeyPool pool;              // bits: clear but for the pad bits; *free_rows: n_rows
    int max_blocks;              // workgroups the launch takes at most (they stride over chunks of 256 x FR_KEYADMIT_PER_THREAD slots)
};
// Each enqueues its one launch on `stream` (a hipStream_t).  -> 0 or the hipError_t value.  An admit is admit, then settle, on one stream.
extern "C" int fr_keyadmit_admit_launch(const FrKeyAdmitArgs *args, void *stream);
extern "C" int fr_keyadmit_settle_launch(const FrKeyAdmitArgs *args, void *stream);
extern "C" int fr_keyadmit_release_launch(const FrKeyReleaseArgs *args, void *stream);
extern "C" int fr_keyadmit_mark_launch(const FrKeyMarkArgs *args, void *stream);

// ---- host objects -------------------------------------------------------------------------------
// Where a table's rows live inside ctx->table_arena.  A table stored on its own: row r at byte_offset + r * dim * 4 (il_rows == 0).
// FR_INDEX_PER_BANK contexts interleave the tables of one memory bank: rows [0, il_rows) of every table of the bank share one
// "bank row" of row_stride bytes (row r of this table at byte_offset + r * row_stride, byte_offset already including the table's
// column offset inside the bank row); rows [il_rows, rows) -- unreachable through a per-bank index, kept so that upload / download /
// fill see the whole table -- sit contiguously at tail_offset.
struct FrTableMem {
    uint64_t byte_offset = 0;  // inside ctx->table_arena: row 0
    uint64_t row_stride = 0;   // bytes between rows [0, il_rows) when interleaved; dim * 4 otherwise
    uint64_t il_rows = 0;      // rows held in the bank-interleaved region (0 = none)
    uint64_t tail_offset = 0;  // inside ctx->table_arena: row il_rows (interleaved tables only)
    bool resident = false;     // false when the table belongs to another shard
};

// (the public headers name the handle types, which gives them default visibility: the destructors that now release things are kept inside the library,
// so that its export list stays what it was -- fr_ctx's has always been in it)
#define FR_HIDDEN_DTOR(type) __attribute__((visibility("hidden"))) ~type() = default
struct fr_ctx {
    int device = -1;
    bool cpu = false;                      // the CPU back-end (fr_ctx_create with device = -1, fr_cpu.cpp): every pointer below is host memory, no HIP call is made
    fr_model_desc model{};                 // deep copy (tables/segments point into the vectors below)
    std::vector<fr_table_desc> tables;
    std::vector<fr_segment> segments;
    std::vector<FrTableMem> table_mem;
    std::vector<int> bank_of_table;        // index column of every table in FR_INDEX_PER_BANK mode (banks numbered by first appearance)
    std::vector<int64_t> bank_rows;        // per bank: min rows over its tables = the valid range of the bank's index
    int n_banks = 0;
    FrBuf<char> table_arena;               // one allocation holding every resident table, 256-B aligned starts
    size_t table_arena_bytes = 0;
    bool tables_filled = false;
    // record geometry
    int n_words = 0;                       // words this ctx gathers per item (whole record, or the shard's slice)
    FrBuf<FrWordDesc> d_words;             // [n_words]
    std::vector<FrWordDesc> h_words;
    FrGatherGroups gather_groups{};        // XCD partition of the record words (gather_pack_xcd_kernel); max_words == 0: none
    // item-tile gather plan (SEMANTIC / sharded layouts): passes grouped in chunks of <= FR_TILE_WORDS record words
    FrBuf<FrPassDesc> d_passes;
    FrBuf<FrChunkDesc> d_chunks;
    int n_chunks = 0;
    // Operand-type bank image (round 6; FR_INDEX_PER_BANK contexts, bf16 / fp8 chains): the reachable rows [0, bank_rows[b]) of every bank
    // once more, already in the chain's operand type -- bf16, or e4m3 at the X exponent -- so that the in-chain gather of a large batch
    // fetches 82 lines per Model-C item instead of 142 and converts nothing.  Made from the fp32 arena by the SAME rounding functions the
    // gather applies (RNE at fill = RNE at gather: bit-identical scores); rebuilt lazily (lp_ensure_image) when the precision, the X exponent
    // or the table contents have changed.  The fp32 arena stays the master (gather_only, fp32 chain, calibration, upload / download).
    std::vector<int> h_word_table, h_word_col;   // per h_words entry: source table (-1: dense) and the float column inside its row
    FrBuf<char> lp_arena;
    FrBuf<FrWordDesc> d_words_lp;          // h_words with src / stride pointing into lp_arena (dense words unchanged)
    int lp_prec = 0, lp_e_x = 0;           // what the image holds (FR_FC_BF16 / FR_FC_FP8 and, for fp8, the X exponent); 0 = nothing
    uint64_t lp_tables_gen = 0;            // tables_gen the image was made from
    uint64_t tables_gen = 1;               // bumped by every fill / upload
    std::mutex lp_mutex;
    // Row updates (fr_worker_update_rows / fr_ctx_update_rows) patch the image in place: where lp_ensure_image put every table, kept under lp_mutex
    struct LpTable {
        size_t base = 0;       // inside lp_arena: (row 0, column 0) of the table
        size_t stride = 0;     // bytes between image rows
        uint64_t rows = 0;     // rows the image holds of it: the bank's common range (FR_INDEX_PER_BANK), the table's own otherwise; 0: not in the image
    };
    std::vector<LpTable> lp_tables;
    std::atomic<long long> lp_builds{0};   // full builds of the image so far (fr_ctx_lp_bank_image_builds); a patch never counts
    // staging of fr_ctx_update_rows (grown on demand, used under lp_mutex on the set-up stream) and its index-range word (pinned, device-visible)
    FrBuf<int32_t> d_up_ids;
    FrBuf<float> d_up_rows;
    FrBuf<int> h_up_err;
    int *d_up_err = nullptr;               // h_up_err's device-side alias
    std::atomic<int> lp_image_on{1};       // fr_ctx_set_lp_bank_image (fleetrec_diag.h): 0 = the in-chain gather reads the fp32 rows and converts them itself
    // Pooled (multi-hot) lookups (fr_ctx_set_pooling): the descriptors made of the hots per index column, P = sum of hots (0: no pooling)
    std::vector<FrPoolDesc> h_pool;
    FrBuf<FrPoolDesc> d_pool;              // [2 * n_words]: the padded form's descriptors, then the offsets form's (d_pool_csr)
    // the offsets (CSR) form's descriptors: first = the word's index COLUMN, hots = the column's cap | FR_POOL_DESC_MEAN
    std::vector<FrPoolDesc> h_pool_csr;
    FrPoolDesc *d_pool_csr = nullptr;      // = d_pool + n_words
    int pool_cols = 0;                     // P
    int pool_max_hots = 0;
    bool pool_wide = false;                // every bag starts and ends on a multiple of 4 slots and P % 4 == 0: 16-byte index loads
    std::vector<int32_t> pool_hots;        // hots per index column, as set
    std::vector<int32_t> pool_modes;       // FR_POOL_SUM / FR_POOL_MEAN per index column (fr_ctx_set_pooling_modes); in the descriptors as FR_POOL_DESC_MEAN
    bool pool_any_mean = false;            // a column is MEAN: the weighted entry points refuse
    // Request-form batches (fr_ctx_set_request_columns): which index columns are the request's, and per form (FR_REQ_*) the per-word
    // descriptor table of the expansion (FrRequestArgs::desc) with its three widths.  Rebuilt when the split or the pooling changes.
    std::vector<int32_t> req_shared;       // [index columns] 0/1; empty: no split is set
    bool req_dense_shared = false;
    struct ReqForm {
        std::vector<int32_t> desc;         // [row_words]; empty: the form is not available
        int req_words = 0, cand_words = 0;
        size_t d_first = 0;                // where the table starts inside d_req_desc
    } req_form[3];
    FrBuf<int32_t> d_req_desc;             // the three tables, one after the other
    // Keyed lookups (fr_ctx_set_key_space): one key space per index column.  `keyed` turns true with the first non-default key space and stays: workers
    // created from then on carry the pinned key rows of the host form.  The records and the word -> column tables a resolve reads live in device memory
    // (plain host memory on the CPU back-end); the tables follow the pooling and the request split, so they are made again, under key_mutex, by the first
    // resolve after either has changed (both change only while no worker has work in flight).
    struct KeySpace {
        int mode = 0;                      // FR_KEYS_ROWS
        uint64_t seed = 0;
        int64_t max_keys = 0;
        int32_t miss_row = 0x7fffffff;
        FrBuf<FrKeySlot> slots;            // MAPPED: the map
        // the row pool (fr_ctx_set_row_pool; pool_rows == 0: none): a rebuild hands it to the new map, fr_ctx_set_key_space drops it with the old one
        int32_t pool_first = 0, pool_rows = 0;
        FrBuf<uint32_t> pool_bits;         // one bit per pool row, set = taken
        FrBuf<int32_t> pool_free;          // [1]: the free rows
        // (moved by std::swap in more than one file: kept inside the library, like the destructors, so that its export list stays what it was)
        KeySpace() = default;
        __attribute__((visibility("hidden"))) KeySpace(KeySpace &&) = default;
        __attribute__((visibility("hidden"))) KeySpace &operator=(KeySpace &&) = default;
    };
    std::vector<KeySpace> key_spaces;      // [index columns]; empty until the first fr_ctx_set_key_space
    bool keyed = false;
    std::vector<FrKeyCol> h_key_cols;      // [index columns]: what d_key_cols holds
    FrBuf<FrKeyCol> d_key_cols;
    FrBuf<uint32_t> d_key_counts;          // [index columns]: keys in every map
    FrBuf<unsigned long long> d_key_walk;  // [3]: the counters of one walk of a map (fr_keymaint.hip); device contexts only, used under key_mutex on the set-up stream
    std::mutex key_mutex;                  // guards the creation of the key spaces (key_spaces_init) and the tables below; the CPU back-end's puts take lp_mutex
    struct KeyTable {
        size_t first = 0;                  // inside d_key_wcol
        int words = 0;                     // W; 0: the form is not available (no split, no pooling)
    } key_tab[3][2];                       // [rows_kind][pooled]
    FrBuf<uint16_t> d_key_wcol;
    std::vector<int32_t> key_tab_hots, key_tab_shared;   // the pooling and the split the tables were made for
    bool key_tab_made = false;
    FrBuf<int64_t> d_kp_keys;              // staging of fr_ctx_put_keys (grown on demand, used under lp_mutex on the set-up stream)
    FrBuf<int32_t> d_kp_rows;
    FrBuf<FrKeySlot> d_ka_tab;             // the call's own table of fr_ctx_admit_keys (grown on demand, used under lp_mutex on the set-up stream)
    std::mutex workers_mutex;              // guards `workers`
    std::vector<struct fr_worker *> workers;   // live workers (fr_ctx_set_pooling asks each whether it has work in flight)
    FrBuf<unsigned long long> d_merged;    // lookups merged by the dedup gather (FR_GATHER_ITEM_TILE_DEDUP_COUNT)
    std::atomic<int> gather_variant{0};    // fr_gather_variant (fr_ctx_set_gather_variant)
    // FC weights: fp32 master copies in the reference's column-major H x K layout
    // (= K-major "Wt[k][h]", cuda_server.c:215) and optional bf16 copies.
    FrBuf<float> d_w[4];
    FrBuf<float> d_wq[3];  // FC1..FC3 re-packed as Wq[k/4][h][k%4] for the 16-byte operand loads
    FrBuf<uint16_t> d_w_bf16[4];
    // fp8 chain: e4m3 q16 copies of FC1..FC3 and the power-of-two exponents (weights per layer; activations X, R1, R2, R3)
    FrBuf<void> d_w_fp8[3];
    FrBuf<void> d_w_fp8h[3];  // the same weights in the "q16h" layout of the non-scaled fp8 MFMA (fr_fused_tile_hs_kernel<2, ...>); fused-eligible models only
    int f8_e_w[3] = {0, 0, 0};
    int f8_e_act[4] = {0, 0, 0, 0};
    float f8_w_rms_gain[3] = {1.0f, 1.0f, 1.0f};  // ||W_l||_F / sqrt(N_l): rms growth of layer l under uncorrelated inputs
    bool f8_calibrated = false;
    FrBuf<uint32_t> d_stats;  // 16 words of reduction scratch (max |x| bits, sum x^2 per tensor)
    bool weights_set = false;
    // Per-layer epilogues (fr_ctx_set_epilogue): fp32 biases of fc[l + 1] values (device memory; host memory on the CPU back-end; empty: no bias)
    // and the hidden layers' activation.  Never rounded to the chain's operand type; set under the rules of fr_ctx_set_weights.
    FrBuf<float> d_bias[4];
    FrBuf<float> d_negzero;                // GPU contexts: max(fc[1..3]) values of -0.0f, the "no bias" operand of the fused kernels' branch-free epilogue forms (v + -0.0f == v)
    bool has_bias[4] = {false, false, false, false};
    int act[4] = {0, 0, 0, 0};             // FR_ACT_*; act[3] stays FR_ACT_NONE
    FrEpi epi(int l) const { return FrEpi{has_bias[l] ? d_bias[l].p : nullptr, act[l] == FR_ACT_RELU ? 1 : 0, 0}; }
    bool any_epi() const { return has_bias[0] || has_bias[1] || has_bias[2] || has_bias[3] || act[0] || act[1] || act[2]; }
    int fc_precision = FR_FC_FP32;
    // sharding
    int shard_rank = 0, n_shards = 1;
    int slice_offset = 0, slice_len = 0, slice_padded = 0;
    std::vector<int> shard_offset, shard_len;  // record range of EVERY shard (floats), for the all-gathered layout
    hipStream_t setup_stream = nullptr;
    // batches one fused streaming launch carries (fr_ctx_set_stream_group): per context; read by every driver thread
    std::atomic<int> stream_group{FR_FUSED_DEFAULT_BATCHES};
    // host-fed blocks of at most this many batches take the stage pipeline instead of the fused kernel (fr_ctx_set_small_block; 0: never)
    std::atomic<int> small_block{0};
    int n_cu = 0;                          // compute units of the device (grid of the persistent fused kernel); set at creation
    int hk_ok = 0;                         // the persistent K-outer fused kernel applies to this context's descriptors; set at creation
    // Lifetime (round 6): one reference for the handle fr_ctx_create gave out, one per live worker and per communicator handle.  fr_ctx_destroy
    // drops the handle's; the context is released by whoever drops the last -- a worker or communicator destroyed AFTER its context no longer
    // walks freed memory (a failed test's teardown did exactly that: "corrupted double-linked list").
    std::atomic<int> life{1};
    std::atomic<int> n_workers{0};         // live workers of the context
    std::atomic<int> worker_seq{0};        // workers ever created on the context: a chain model's k-th worker takes the highest (k even) / lowest (k odd) stream priority
    // chain width W (fr_ctx_set_chain_width): the bf16 / fp8 GEMM layers of a chain model take tiles that cover 1 / W of the chip (lp_gemm_mu).
    // 0 = not decided yet: the first low-precision GEMM-layer launch on the context freezes it at min(live workers, 4); from then on only an
    // explicit fr_ctx_set_chain_width changes it -- never a worker coming or going
    std::atomic<int> chain_width{0};
    std::atomic<bool> chain_width_auto{false};   // the width was frozen by a launch (not by fr_ctx_set_chain_width / a driver): fr_worker_create leaves a note when workers outnumber it
};

struct fr_worker {
    FR_HIDDEN_DTOR(fr_worker);
    fr_ctx *ctx = nullptr;
    int max_batch = 0;
    int idx_cap = 0;             // int32 columns per item its pinned and device index buffers hold: max(index columns, pooled columns at creation)
    FrBuf<float> h_pool_w;       // pinned [max_batch][pool_w_cap] per-sample weights of the host form (fr_worker_pool_weights_ptr); NULL without pooling at creation
    int pool_w_cap = 0;          // pooled columns at creation
    FrBuf<int32_t> h_pool_off;       // pinned [max_batch * index columns + 1] bag offsets of the offsets-form host call (fr_worker_pool_offsets_ptr); NULL without pooling at creation
    // Request-form host call (fr_worker_submit_requests): the request side's pinned buffers, there on a worker created after fr_ctx_set_request_columns
    FrBuf<int32_t> h_req_idx;        // [max_batch][req_idx_cap]
    FrBuf<float> h_req_w;            // [max_batch][req_w_cap]; NULL without pooling at creation
    FrBuf<float> h_req_dense;        // [max_batch][dense_len]; NULL unless dense_shared
    FrBuf<int32_t> h_req_off;        // [max_batch + 1]
    int req_idx_cap = 0, req_w_cap = 0;   // request words per request at creation: max(Rs, Rs') and Rs'
    FrBuf<float> d_pool_w;           // [max_batch][pool_w_cap]: the expanded per-sample weights (host memory on the CPU back-end)
    // Keyed lookups: the pinned key rows of the host form (fr_worker_key_ptr), there on a worker created after the context's first non-default key space;
    // the counter of MAPPED lookups that found no key (device memory; made by the worker's first resolve)
    FrBuf<int64_t> h_keys;           // [max_batch][idx_cap]
    FrBuf<unsigned long long> d_key_miss;
    FrBuf<FrKeySlot> d_admit_tab;    // the call's own table of fr_worker_admit_keys (device workers; grown on demand by the largest admit so far)
    // CPU back-end: a call computes before it returns; an index-range error stays in c_err until fr_worker_sync reports it
    FrBuf<float> c_scratch;      // [max_batch][H1 + H2 + H3]
    FrBuf<float> c_x;            // records of the sharded FC entry points, [max_batch][K]
    int c_err = 0;
    double c_t0 = 0.0;           // fr_worker_timer_start (steady clock, seconds)
    hipStream_t stream = nullptr;
    // pinned host staging (cudaMallocHost in the reference, cuda_server.c:136-160)
    FrBuf<int32_t> h_idx;
    FrBuf<float> h_dense;
    FrBuf<float> h_score;
    // device buffers (cudaMalloc in the reference, cuda_server.c:170-183)
    FrBuf<int32_t> d_idx;
    FrBuf<float> d_dense;
    FrBuf<float> d_records;     // [max_batch][K]
    // feature-major activations, two sets alternating by launch parity; per set:
    //   Xt[K][ld] | R1t[2][H1][ld] | R2t[2][H2][ld] | R3t[2][H3][ld]   ([2] = K-split partials)
    FrBuf<float> d_act[2];
    int ld_max = 0;             // round_up(max_batch, 64)
    // software pipeline over consecutive batches: slot of the batch whose gather ran in launch L is ring[L % 8]
    struct Slot {
        bool active = false;
        uint64_t launch0 = 0;   // launch number of its stage 0
        int first_stage = 0;    // 0 normally; 1 for fc_only (activations supplied by a transpose)
        int batch = 0, ldm = 0;
        const int32_t *d_idx = nullptr;
        const float *d_dense = nullptr;
        float *d_scores = nullptr;
    } ring[8];
    uint64_t launch_no = 0;     // number of pipeline launches issued so far
    int n_active = 0;
    bool counted = false;       // in fr_ctx::n_workers
    bool diag_launch = false;   // fr_worker_fc_layer_only: a single-layer diagnostic launch reads the chain width it WOULD run at and freezes nothing
    bool calibrating = false;   // fr_worker_calibrate_fp8: the pushed batch runs the fp32 stages without K-split partials
    int last_x_parity = 0;      // which activation set holds Xt of the most recently pushed batch (debug hook)
    // fused item-tile path: batches queued by fr_worker_push_device until a launch group is full
    FrFusedBatch pending[FR_FUSED_MAX_QUEUE];
    int n_pending = 0;
    // batch lists of the persistent kernel's launches: FR_BLIST_RING pinned host blocks + device copies, one H2D copy per launch on the
    // worker's stream; a block is rewritten only after the copy that read it has executed (its event)
    FrBuf<FrFusedBatch> h_blist, d_blist;
    FrEvent ev_blist[FR_BLIST_RING];
    bool blist_busy[FR_BLIST_RING] = {false, false, false, false};
    int blist_cur = 0;
    int64_t pending_items = 0;
    FrBuf<float> d_score;
    // host-fed streaming (fr_worker_push_host): FR_HOST_BLOCKS staging blocks of `g` batches each; a block is filled by CPU copies
    // into pinned memory, then moves as ONE H2D copy + ONE fused launch + ONE D2H copy; its event says when the scores are home
    struct HostRing {
        FR_HIDDEN_DTOR(HostRing);
        int g = 0;                 // batches per block (fixed when the ring is created)
        size_t idx_slot = 0, dense_slot = 0, score_slot = 0;  // elements per batch slot
        FrBuf<int32_t> h_idx, d_idx;
        FrBuf<float> h_dense, d_dense, h_sc, d_sc;
        FrEvent ev[4];
        hipStream_t copy = nullptr;   // the blocks' H2D copies run here, ahead of the launches on the worker's stream (ev_in: block b's rows have landed)
        FrEvent ev_in[4];
        bool inflight[4] = {false, false, false, false};
        int count[4] = {0, 0, 0, 0};          // batches in the block
        float *dst[4][FR_FUSED_MAX_BATCHES];  // where each batch's scores go
        int bsz[4][FR_FUSED_MAX_BATCHES];
        int cur = 0;               // block being filled
        int staged = 0;            // batch size handed out by fr_worker_stage_acquire and not yet pushed (0: none)
        long long delivered = 0;   // host-fed batches whose scores have been copied to their h_scores so far (fr_worker_host_poll)
    } hr;
    // table-sharded exchange (fr_worker_submit_sharded, fr_comm.cpp): this shard's slice, the all-gathered slices, score chunks
    FrBuf<void> d_slice, d_gathered;
    FrBuf<float> d_score_part, d_score_all;  // [chunk + 1], [G][chunk + 1]: every rank's chunk ends with its status word
    FrBuf<float> h_sh_status;  // pinned: [0] this rank's status word as sent, [1 .. G] the status words of all ranks as received
    struct fr_comm *sh_comm = nullptr;  // a sharded step is in flight through this communicator (fr_worker_sync -> fr_comm_wait)
    int sh_ranks = 0;
    std::atomic<int> sh_inject_fc_fail{0};   // fr_worker_inject_fc_failure (fleetrec_diag.h): sharded steps left whose FC chain is reported as failed
    FrBuf<void> h_stage_send, h_stage_recv;   // pinned staging of the STAGED host exchange (GPU shard contexts that share a device)
    void *sh_host_stream = nullptr;  // CPU workers: the host stream their sharded steps run on (fr_comm.cpp HostStream), made on first use
    FrBuf<int> err_word;   // sticky index-range flag: the pinned, device-visible host word of a GPU worker (a CPU worker's is c_err) ...
    int *h_err = nullptr;  // ... as the host reads it ...
    int *d_err = nullptr;  // ... and its device-side alias
    bool in_flight = false;
    // fr_worker_update_rows: recorded on the stream behind the update's launches; a rebuild of the operand-type bank image makes the set-up
    // stream wait for it (lp_ensure_image).  Both touched under fr_ctx::lp_mutex only.
    FrEvent ev_update;
    bool update_recorded = false;
    // Segmented top-K ranking (fr_worker_topk_device / fr_worker_topk).  d_rank: the scratch of segments longer than FR_RANK_PART (head, unit records,
    // candidate lists), allocated by the first call over more than FR_RANK_PART scores, grown (behind a wait for the stream) when a call needs more.
    FrBuf<char> d_rank;
    int host_batch = 0;          // items of the host-form batch in flight (fr_worker_submit, the three host-form pooled submits); 0: none
    // host form: pinned staging of the offsets and of the results, which fr_worker_sync copies to where the caller wants them
    FrBuf<int32_t> h_tk_off, h_tk_idx;
    FrBuf<float> h_tk_sc;
    int32_t *tk_dst_idx = nullptr;
    float *tk_dst_sc = nullptr;
    size_t tk_count = 0;         // n_seg * k of the host-form ranking in flight; 0: none
    char last_kernel[96] = "";  // fr_worker_last_kernel: the dominant kernel of the most recent launch this worker enqueued
    FrEvent ev_start, ev_stop;
};

size_t idx_cols(const fr_ctx *c);   // int32 index columns per item of a one-hot batch (fr_api.cpp)
// refusals fr_api.cpp and fr_comm.cpp share (fr_api.cpp): no pooling set (always fails; its three texts: an unsharded context or a host form, a shard on
// an unsharded entry point, the sharded step), weights against a FR_POOL_MEAN column, the two ends of `who`'s pinned bag offsets (*nnz = the last)
enum FrNoPooling { FR_NO_POOLING_PLAIN, FR_NO_POOLING_SHARD, FR_NO_POOLING_SHARDED_STEP };
int fr_pooling_unset(FrNoPooling who);
int fr_pooled_weights_need_sum(const fr_ctx *c);
int fr_pooled_host_offsets(const fr_worker *w, int batch, const char *who, int64_t *nnz);
void fr_ctx_ref(fr_ctx *c);     // + 1 reference (a worker, a communicator handle)
void fr_ctx_unref(fr_ctx *c);   // - 1; the last one releases the context
inline FrMem fr_mem_kind(const fr_ctx *c, FrMem k) { return c->cpu ? FrMem::HOST : k; }

// ---- table-sharded exchange (fr_comm.cpp) ------------------------------------------------------------
int fr_comm_wait(fr_worker *w);  // bounded wait for the sharded step in flight + the ranks' status words; FR_OK when none is in flight
bool fr_comm_step_on_host_stream(const fr_worker *w);   // a sharded step of this worker is being issued by its host stream right now
void fr_comm_worker_release(fr_worker *w);  // fr_worker_destroy of a CPU worker: stop its host stream (bounded), then fr_comm_forget
void fr_comm_forget(fr_worker *w);  // drop the step's hold on its communicator without waiting (fr_worker_sync leaving early)

// ---- CPU back-end (fr_cpu.cpp): device = -1 -----------------------------------------------------------
int frc_set_threads(int n);   // 0: all usable cores; -> the pool's size
int frc_threads();
void *frc_arena_alloc(size_t bytes);   // nullptr (+ fr_last_error) when the host cannot hold it
void frc_arena_free(void *p, size_t bytes);
int frc_fill_table(float *base, int64_t row0, int64_t rows, int dim, int64_t row_stride_bytes, int mode, uint32_t seed, uint32_t uid);
int frc_fill_weights(float *w, size_t count, int mode, uint32_t seed, uint32_t layer, float scale);
int frc_gather(const FrWordDesc *words, int n_words, const int32_t *idx, int idx_stride, const float *dense, float *out, int batch, int *err_flag);
int frc_gather_pooled(const FrPooledPlan &p, const FrPooledBatch &b, const FrPooledOut &o);   // fp32 records only (FrPooledOut::RECORDS)
// n listed rows of one table <- src [n][dim], into the host arena with table_copy's head / tail addressing, over the pool's threads; a listed
// id outside [0, rows) writes nothing and -> 1 (else 0).  A row listed twice ends up as the LAST of its listed sources.
int frc_update_rows(char *arena, const FrTableMem &tm, int dim, int64_t rows, int n, const int32_t *ids, const float *src);
// the CPU twin of fr_rank_launch: the same outputs bit for bit, segments over the pool's threads; -> 1 when a segment was malformed (ranked as empty), else 0
int frc_rank_topk(const float *scores, int n, int n_seg, const int32_t *off, int k, int32_t *top_idx, float *top_scores);
// the CPU twin of fr_request_launch: the same words, items over the pool's threads; -> 1 when the offsets were malformed, else 0
int frc_expand_requests(const FrRequestArgs &a);
// the CPU twins of fr_key_resolve_launch (words over the pool's threads), fr_key_put_launch (pair after pair, ONE writer at a time -- the callers hold
// fr_ctx::lp_mutex; readers need no lock: the key is published before the row --: of a key listed twice the last row stays;
// -> the FR_KEYS_ERR_* bits of the pairs that were not applied) and fr_key_fill_launch
void frc_resolve_keys(const FrKeyResolveArgs &a);
int frc_put_keys(const FrKeyPutArgs &a);
void frc_fill_keys(const FrKeyFillArgs &a);
// the CPU twins of fr_keymap_erase_launch (-> FR_KEYS_ERR_ERASE_EMPTY or 0; the callers hold fr_ctx::lp_mutex) and fr_keymap_walk_launch (one pass,
// slot after slot, the same fr_keys.h predicates; export order: by slot)
int frc_erase_keys(const FrKeyEraseArgs &a);
void frc_walk_keys(const FrKeyWalkArgs &a);
// the CPU twins of fr_keyadmit_admit_launch + _settle_launch (key after key, the LOWEST free row first; -> the FR_KEYS_ERR_* bits of the keys that were
// not applied), fr_keyadmit_release_launch (-> FR_KEYS_ERR_ERASE_EMPTY or 0) and fr_keyadmit_mark_launch; the callers hold fr_ctx::lp_mutex
int frc_admit_keys(const FrKeyAdmitArgs &a);
int frc_release_keys(const FrKeyReleaseArgs &a);
void frc_mark_pool(const FrKeyMarkArgs &a);
void frc_fc_chain(const int32_t fc[5], const float *const w[4], const FrEpi epi[4], const float *X, int batch, float *scratch, float *scores);
void frc_slices_to_records(const float *gathered, int n_shards, int batch_total, int slice_padded, const int *offs, const int *lens, int item0, int n_items, float *X, int K);
// every entry point selects its context's device first; a CPU context (device = -1, fr_cpu.cpp) has none
#define FR_SET_DEVICE(ctx_)                                    \
    do {                                                       \
        if (!(ctx_)->cpu) FR_HIP(hipSetDevice((ctx_)->device)); \
    } while (0)

// ---- the seams between fr_api.cpp and fr_keyspace.cpp -------------------------------------------------------------------------------
// fr_api.cpp's, called by the keyed code:
int fr_pooling_busy(fr_ctx *ctx, const char *who);           // refuses while a worker of the context has work in flight
int fr_fused_flush(fr_worker *w);                            // launches the batches queued for a fused launch, without waiting
int fr_host_fed_queued(fr_worker *w, const char *verb);      // refuses while host-fed batches wait in a block not launched yet: "... flush first ..., then <verb>"
int fr_up_err_ensure(fr_ctx *ctx);                           // the set-up stream's status word (h_up_err / d_up_err), made on first use; under lp_mutex
int fr_up_err_take(fr_ctx *ctx);                             // ... read and cleared
// fr_keyspace.cpp's, called by fr_worker_sync and fr_worker_submit_keyed:
int fr_index_range_fail(int bits);                           // FR_ERR_INDEX_RANGE with the text of a status word's bits (bit 0: a lookup; FR_KEYS_ERR_*)
int fr_key_unsharded(const fr_ctx *c, const char *who);      // refuses a sharded context
int fr_key_resolve_enqueue(fr_worker *w, int n_rows, int rows_kind, int pooled, const int64_t *keys, int32_t *out, const char *who);   // the one resolve launch

#define FR_NOT_ON_CPU(ctx_, what)                                                                                                  \
    do {                                                                                                                           \
        if ((ctx_)->cpu) FR_FAIL(FR_ERR_STATE, "%s is not available on the CPU back-end (device = -1): fp32 submit / sync / gather_only / fc_only only", what); \
    } while (0)

// ---- registry (fr_registry.cpp) -------------------------------------------------------------------
int fr_model_validate(const fr_model_desc *m);

// ---- kernel launchers (fr_*.hip) -------------------------------------------------------------------
// uid used by the procedural fills: source*1024 + class*256 + table_id
static inline uint32_t fr_table_uid(const fr_table_desc &t) {
    return (uint32_t)t.source * 1024u + (uint32_t)t.mem_class * 256u + (uint32_t)t.table_id;
}
int frk_fill_table(float *base, int64_t row0, int64_t rows, int dim, int64_t row_stride_bytes, int mode, uint32_t seed, uint32_t uid, hipStream_t s);
int frk_fill_weights(float *w, size_t count, int mode, uint32_t seed, uint32_t layer, float scale, hipStream_t s);
// rows [0, rows) of an fp32 region (row r at src + r * src_stride, `floats` floats wide) -> the same rows in the operand type of `precision`
// (bf16: RNE; fp8: x 2^e_x, saturated, e4m3) at dst + r * dst_stride: the rounding of the gather kernels themselves (fr_device.h)
// ids != NULL: the `rows` listed rows ids[0 .. rows) instead, those inside [0, image_rows) (the patch behind fr_worker_update_rows)
int frk_convert_rows_lp(int precision, const void *src, size_t src_stride, void *dst, size_t dst_stride, int64_t rows, int floats, int e_x, hipStream_t s,
                        const int32_t *ids = nullptr, int64_t image_rows = 0);
// fill_table_kernel's "rows from a list" arm: n listed rows ids[n] of one table <- src [n][dim]; head / tail: rows [0, head_rows) at `head`
// (row_stride_bytes apart), rows [head_rows, rows) dense at `tail`; an id outside [0, rows) raises *err_flag (system-scope) and writes nothing
int frk_scatter_rows(float *head, int64_t row_stride_bytes, float *tail, int64_t head_rows, int64_t rows, int dim, int n, const int32_t *ids, const float *src, int *err_flag,
                     hipStream_t s);
int frk_gather(const FrWordDesc *words, int n_words, const FrGatherGroups &groups, const int32_t *idx, int idx_stride, const float *dense, void *out, int batch, int *err_flag,
               int transport, int e_x, hipStream_t s, int out_words, bool one_chunk = false);
// pooled (multi-hot) gather of the batch `b` (padded or offsets form) by the descriptors of `p` into `o`, one launch on `s`
// -> FR_POOL_NO_OPERAND_ARM (nothing launched) when `o` is the chain's OPERAND and the shape this batch takes has no operand-store arm: the caller writes
// records and converts them.  An LP_SLICE without the arm takes the neighbouring shape instead, so that call never returns FR_POOL_NO_OPERAND_ARM.
int frk_gather_pooled(const FrPooledPlan &p, const FrPooledBatch &b, const FrPooledOut &o, hipStream_t s);
int frk_gather_tile(const FrPassDesc *passes, const FrChunkDesc *chunks, int n_chunks, const int32_t *idx, int idx_stride, const float *dense, void *out,
                    int out_stride_words, int batch, int *err_flag, bool dedup, unsigned long long *dup_counter, hipStream_t s);
int frk_transpose_slices_lp(int precision, const void *gathered, int n_shards, int batch_total, int slice_padded, const int *h_offsets, const int *h_lens,
                            int item0, int n_items, void *X, int K, int ldm, hipStream_t s);
// feature-major FC chain, stage-pipelined across batches (see fr_pipeline.hip)
int frk_pipeline_launch(const FrPipeArgs &a, int single_stage, int precision, hipStream_t s);
int frk_pack_weights_q8_bf16(const float *W, uint16_t *Wh, int K, int H, hipStream_t s);
bool frk_fc_lp_gemm_ok(int precision, int K, int N, int ldm);
// width: the context's chain width (fr_ctx::chain_width) -> the larger tile already when it covers 1 / width of the chip (lp_gemm_mu)
int frk_fc_lp_gemm(int precision, const void *Wp, const void *Xp, void *Yp, int K, int N, int ldm, int e_w, int e_in, int e_out, int width, bool minor, const FrEpi &epi, hipStream_t s);   // epi: the layer's epilogue
bool frk_fused_hk_takes_lp_rows(int K);   // the persistent bf16 fused kernel has an instantiation that reads operand-type (bf16) rows for this record length
bool frk_fc_tail_ok(int precision, int K, int N, int ldm);   // FC3 + output layer as one launch (fc_tail_kernel, fr_gemm.hip)
int frk_fc_tail(int precision, const void *W3, const void *R2, const void *wout, float *scores, int K, int N, int ldm, int batch, int e_w, int e_in, int e_r3, const FrEpi &epi3, const FrEpi &epi_out,
                hipStream_t s);   // epi3: FC3's epilogue, applied before R3 is rounded in registers; epi_out: b_3
int frk_records_to_q8_bf16(const float *X, void *Xh, int batch, int K, int ldm, hipStream_t s);
int frk_pack_weights_q16_fp8(const float *W, void *Wf, int K, int H, int e_w, hipStream_t s);
int frk_pack_weights_q16h_fp8(const float *W, void *Wg, int K, int H, int e_w, hipStream_t s);  // the persistent fp8 kernel's operand layout
int frk_records_to_q16_fp8(const float *X, void *Xf, int batch, int K, int ldm, int e_x, hipStream_t s);
// ldm > 0: p is a feature-major q4 image [n / 4 / ldm][ldm][4] and only the items m < batch count (the pad items of a chain with biases are not zeros)
int frk_stats(const float *p, size_t n, void *d_out, hipStream_t s, int ldm = 0, int batch = 0);
int frk_q4_to_lp(int precision, const float *Xq, void *Xo, int K, int ldm, int e_x, hipStream_t s);
int frk_stage_blocks_f8_gather(int K, int ldm);
int frk_pack_weights_q4(const float *W, float *Wq, int K, int H, hipStream_t s);
int frk_stage_blocks(int stage, int n_words, int K, int N, int ldm, int nsplit);
int frk_gather_tr_blocks(int n_words, int ldm, int variant);
int frk_gather_tr_variant(int batch, int idx_stride);
bool frk_fused_ok(int K, int H1, int H2, int H3);
int frk_fused_launch(const FrFusedArgs &a, hipStream_t s);
bool frk_fused_m2_ok(int K, int H1, int H2, int H3);
int frk_fused_m2_launch(const FrFusedArgs &a, hipStream_t s);
bool frk_fused_h_ok(int K, int H1, int H2, int H3);
bool frk_fused_f8_ok(int K, int H1, int H2, int H3);
int frk_fused_f8_launch(const FrFusedArgs &a, hipStream_t s);
int frk_fused_h_items_per_wg();
int frk_fused_h_launch(const FrFusedArgs &a, hipStream_t s);
bool frk_fused_hk_ok(int K, int H1, int H2, int H3, const FrWordDesc *h_words, int n_words);  // the K-outer persistent kernel (fr_fused_ko.hip), bf16 and fp8 forms
int frk_fused_hk_launch(const FrFusedArgs &a, int n_cu, int precision, hipStream_t s);  // 0 when the transposing gather does not apply
int frk_transpose_records(const float *X, float *Xt, int batch, int K, int ldm, hipStream_t s);
int frk_transpose_slices(const float *gathered, int n_shards, int batch_total, int slice_padded, const int *h_offsets, const int *h_lens,
                         int item0, int n_items, float *Xq, int ldm, hipStream_t s);
void fr_shard_bounds(const fr_model_desc &m, int n_shards, std::vector<int> &seg_begin);
// memory banks of the model: bank key = (source, mem_class, bank); numbered by first appearance in the table list
int fr_bank_map(const fr_model_desc &m, std::vector<int> &bank_of_table, std::vector<int64_t> &bank_min_rows);

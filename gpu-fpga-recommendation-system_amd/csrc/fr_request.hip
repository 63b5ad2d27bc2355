// Request-form batches (fr_worker_expand_requests_device / fr_worker_submit_requests, fleetrec_serving.h) -> libfleetrec_request.so, the second
// COMPANION code object of libfleetrec.so, built and linked as libfleetrec_rank.so is (the kernel list of libfleetrec.so is pinned name for name, and
// the ranking companion's kernels all carry rank_ in their names).  It calls nothing of libfleetrec.so: its one launcher returns a hipError_t value.
//
// request_expand_kernel: a batch arrives as request rows [n_req][Rs] + candidate rows [batch][Rc] + segment offsets [n_req + 1]; the kernel writes
// the full rows [batch][W] every existing lookup path takes.  A workgroup of 256 threads expands a tile of g.tile <= 64 consecutive items:
//   1. thread t < items of the tile finds the request that owns item i0 + t -- the last r with off[r] <= i, a binary search over off[0 .. n_req),
//      CLAMPED into [0, n_req) whatever the array holds -- and leaves it in LDS: once per item, not once per word;
//   2. the tile's output words, one contiguous run out[i0 * W .. (i0 + items) * W), are dealt to the threads in order: every wave-instruction
//      stores 64 consecutive dwords (256 bytes), whatever W is (Model-A's rows are 188 bytes: no 16-byte row start is assumed, no access is
//      wider than a dword).  Word w of a row takes its source from the descriptor table: desc[w] >= 0 -> cand[i * Rc + desc[w]], desc[w] < 0 ->
//      req[owner * Rs + ~desc[w]].  (item, word) advance by (256 / W, 256 % W) per step: no division inside the loop.
// Validation rides in the same launch: thread j of the grid checks off[j] <= off[j + 1] (grid-stride over the n_req pairs), thread 0 of workgroup
// 0 the two ends; a violation raises the worker's index-range word.
// Bounds, for ANY content of off: owner is in [0, n_req) by the clamp and ~desc[w] < Rs, desc[w] < Rc by construction of the table (fr_api.cpp,
// request_prepare), so req is read inside [0, n_req * Rs), cand inside [0, batch * Rc) (i < batch), off inside [0, n_req], and out is written
// inside [0, batch * W).  Every word written is a copy of a word of req or cand.
#include <hip/hip_runtime.h>

#include "fr_internal.h"

__global__ __launch_bounds__(256) void request_expand_kernel(const FrRequestArgs g) {
    __shared__ int s_owner[FR_REQ_TILE_MAX];
    const int tid = (int)threadIdx.x;
    const int i0 = (int)blockIdx.x * g.tile;   // < batch <= 2^24
    const int items = g.batch - i0 < g.tile ? g.batch - i0 : g.tile;
    if (g.off) {
        bool bad = false;
        const size_t step = (size_t)gridDim.x * 256u;
        for (size_t j = (size_t)blockIdx.x * 256u + (size_t)tid; j < (size_t)g.n_req; j += step) bad |= g.off[j] > g.off[j + 1];
        if (blockIdx.x == 0 && tid == 0) bad |= g.off[0] != 0 || g.off[g.n_req] != g.batch;
        if (bad) atomicOr_system(g.err_flag, 1);   // pinned host word; error path only
    }
    if (tid < items) {
        const int i = i0 + tid;
        int r;
        if (g.off) {   // lo = how many of off[0 .. n_req) are <= i, were the array sorted; any array leaves lo in [0, n_req]
            int lo = 0, hi = g.n_req;
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if (g.off[mid] <= i) lo = mid + 1;
                else hi = mid;
            }
            r = lo - 1;
        } else {
            r = i / (g.batch / g.n_req);   // (the host refused batch % n_req != 0: n_req <= batch)
        }
        s_owner[tid] = r < 0 ? 0 : (r >= g.n_req ? g.n_req - 1 : r);
    }
    __syncthreads();
    const int W = g.W;
    const unsigned total = (unsigned)items * (unsigned)W;   // <= 64 x 376 x 64
    uint32_t *out = g.out + (size_t)i0 * (size_t)W;
    int item = tid / W, word = tid % W;
    const int d_item = 256 / W, d_word = 256 % W;
    for (unsigned e = (unsigned)tid; e < total; e += 256u) {
        const int d = g.desc[word];
        out[e] = d >= 0 ? g.cand[(size_t)(i0 + item) * (size_t)g.Rc + (size_t)d] : g.req[(size_t)s_owner[item] * (size_t)g.Rs + (size_t)(~d)];
        item += d_item, word += d_word;
        if (word >= W) word -= W, item++;
    }
}

extern "C" __attribute__((visibility("default"))) int fr_request_launch(const FrRequestArgs *args, void *stream) {
    const FrRequestArgs g = *args;
    const unsigned blocks = (unsigned)((g.batch + g.tile - 1) / g.tile);
    request_expand_kernel<<<dim3(blocks), dim3(256), 0, (hipStream_t)stream>>>(g);
    return (int)hipGetLastError();
}

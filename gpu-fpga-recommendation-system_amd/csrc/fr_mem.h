// Who owns a buffer (included by fr_internal.h; host-only C++: no __device__ code, nothing here reaches a code object).  Every allocation of the
// contexts, workers and drivers goes through fr_mem_alloc / fr_mem_release (fr_api.cpp) and is held by an FrBuf, which releases it by its kind
// when its owner is deleted; the events are held by FrEvent.  Streams stay explicit: they are synchronised before anything is released.
#pragma once

#include <cstddef>
#include <cstdint>
#include <utility>

// HOST: 64-byte-aligned aligned_alloc, the size rounded up to 64 (0 bytes: 64).  ARENA: the CPU back-end's table arena (frc_arena_alloc).
enum class FrMem : uint8_t { HOST, PINNED, PINNED_MAPPED, DEVICE, ARENA };
struct fr_ctx;
FrMem fr_mem_kind(const fr_ctx *c, FrMem k);   // the kind a context's buffer takes: on the CPU back-end (ctx->cpu) every kind is HOST
// -> FR_OK, FR_ERR_OOM (hipErrorOutOfMemory, a failed aligned_alloc) or FR_ERR_HIP; fr_last_error() names `what`.  *out is NULL on failure.
int fr_mem_alloc(FrMem kind, size_t bytes, const char *what, void **out);
void fr_mem_release(FrMem kind, void *p, size_t bytes);
// live bytes held through the two functions above, process-wide: [0] device memory, [1] host memory (pinned; the CPU back-end's plain stand-ins)
void fr_mem_live_bytes(uint64_t out[2]);

template <class T> struct FrElem { static constexpr size_t size = sizeof(T); };
template <> struct FrElem<void> { static constexpr size_t size = 1; };

template <class T> struct FrBuf {   // move-only: pointer, element count, kind
    T *p = nullptr;
    size_t n = 0;
    FrMem kind = FrMem::HOST;
    FrBuf() = default;
    FrBuf(const FrBuf &) = delete;
    FrBuf &operator=(const FrBuf &) = delete;
    FrBuf(FrBuf &&o) noexcept { swap(o); }
    FrBuf &operator=(FrBuf &&o) noexcept {
        reset();
        swap(o);
        return *this;
    }
    ~FrBuf() { reset(); }
    operator T *() const { return p; }
    size_t count() const { return n; }
    int alloc(FrMem k, size_t count, const char *what) {   // whatever it held is released first; empty when the allocation fails
        reset();
        const int rc = fr_mem_alloc(k, count * FrElem<T>::size, what, (void **)&p);
        if (rc == 0) n = count, kind = k;
        return rc;
    }
    int grow(FrMem k, size_t count, const char *what) { return p && count <= n ? 0 : alloc(k, count, what); }
    void reset() {
        if (p) fr_mem_release(kind, p, n * FrElem<T>::size);
        p = nullptr, n = 0;
    }
    void swap(FrBuf &o) {
        std::swap(p, o.p);
        std::swap(n, o.n);
        std::swap(kind, o.kind);
    }
};

struct FrEvent {   // an event of the worker's device, destroyed with its owner
    hipEvent_t e = nullptr;
    FrEvent() = default;
    FrEvent(const FrEvent &) = delete;
    FrEvent &operator=(const FrEvent &) = delete;
    ~FrEvent() {
        if (e) (void)hipEventDestroy(e);
    }
    operator hipEvent_t() const { return e; }
    hipError_t create(unsigned flags) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
};

// rtx_devmem.hpp — the owning types of the host runtime: device and pinned memory, the context's events, its borrowed streams.  Every one frees what it holds in its
// destructor, so a context or a builder is released by destroying it; the destructors run with the owner's device bound (rtx_destroy binds it before `delete`, local
// buffers live inside calls that did).  Besides rtx_staging.hpp's pinned chunks, nothing else in the library allocates, frees or destroys these resources.
#pragma once
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <mutex>
#include <vector>

namespace rtx {

// RTX_DEBUG_POISON=<byte> in the environment (tooling: the hunt for reads of memory no kernel of the frame wrote): every fresh device allocation is filled with that byte —
// 255 makes stale floats NaN and stale indices huge, 127 large finite values — so that a result which depends on what a previous context (or process) left in HBM turns
// from a once-in-20 000 mismatch into a reproducible one.  Unset (the product): allocations stay as hipMalloc returns them.
inline int poison_byte() { static const int b = [] { const char* e = getenv("RTX_DEBUG_POISON"); return e && *e ? atoi(e) & 255 : -1; }(); return b; }

// One allocation of device (DevBuf) or pinned host (PinnedBuf) memory.  Move-only; a move assignment frees the target's old memory first.
template <bool kPinned> struct OwnedMem {
    void* p = nullptr; size_t bytes = 0;
    OwnedMem() = default;
    OwnedMem(const OwnedMem&) = delete; OwnedMem& operator=(const OwnedMem&) = delete;
    OwnedMem(OwnedMem&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    OwnedMem& operator=(OwnedMem&& o) noexcept { if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~OwnedMem() { release(); }
    // at least n bytes: nothing happens while they fit; otherwise the old memory is freed (its contents are NOT kept) and n bytes (16 for n = 0) are allocated
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        release();
        if (!n) n = 16;
        hipError_t e = kPinned ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
        if (e == hipSuccess) { bytes = n; if (!kPinned && poison_byte() >= 0) { e = hipMemset(p, poison_byte(), n); if (e == hipSuccess) e = hipDeviceSynchronize(); } }     // (the fill runs on the null stream, the context's streams are non-blocking: join before anything is uploaded)
        return e;
    }
    void release() { if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p)); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};
using DevBuf = OwnedMem<false>;
using PinnedBuf = OwnedMem<true>;

// The events of a context: begin / end of a frame, and a pool that kernel timing and stream joins take from (rewound per frame).  A failed creation leaves a null event,
// which the callers check.
struct Events {
    hipEvent_t begin = nullptr, end = nullptr;
    std::vector<hipEvent_t> pool; size_t used = 0;
    Events() = default; Events(const Events&) = delete; Events& operator=(const Events&) = delete;
    ~Events() { for (hipEvent_t ev : pool) (void)hipEventDestroy(ev); if (begin) (void)hipEventDestroy(begin); if (end) (void)hipEventDestroy(end); }
    hipEvent_t take() {
        if (used == pool.size()) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) return nullptr; pool.push_back(e); }
        return pool[used++];
    }
};

// Streams are BORROWED from a process-wide pool and returned idle; the library never calls hipStreamDestroy.  Round 5 (profiles/r05_determinism.md): in a process that creates
// and destroys thousands of contexts, once in ~700 contexts two words of a live 912-byte heap block — a mesh's index array, the builder's leaf order — changed during a later
// rtx_commit_scene: a write through a stale pointer by code OUTSIDE this library (with the library's own allocations of that size on fenced pages, nothing of ours touched freed
// memory and nothing of ours was hit).  Not releasing events, device or pinned memory left the rate unchanged; not destroying the two streams of a context made it vanish
// (0 findings in 5 500 x 2 contexts against 25 in 17 700 x 2).  A pooled stream also saves the ~50 us its creation costs.
// A context borrows a SET of five streams (its own, the shadow-overlap stream, ReSTIR lanes 1 .. 3) that were created back to back: the runtime spreads streams over its
// (four) hardware queues in creation order, so the streams of one set run concurrently — two streams picked from a pool one by one may share a queue and serialise
// (measured: the two-lane ReSTIR frame of the atrium 8.08 -> 9.82 ms with single pooled streams, kernel times unchanged).
struct StreamSet { int device = -1; hipStream_t s[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; };
struct StreamPool {
    std::mutex mu; std::vector<StreamSet> idle;
    hipError_t acquire(int device, StreamSet& out) {        // the caller has the device bound
        std::lock_guard<std::mutex> g(mu);
        for (size_t i = 0; i < idle.size(); i++) if (idle[i].device == device) { out = idle[i]; idle.erase(idle.begin() + (long)i); return hipSuccess; }
        out = StreamSet(); out.device = device;
        for (hipStream_t& st : out.s) { const hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking); if (e != hipSuccess) return e; }
        return hipSuccess;
    }
    void release(StreamSet& set) {
        if (set.device < 0) return;
        for (hipStream_t st : set.s) if (st) (void)hipStreamSynchronize(st);
        std::lock_guard<std::mutex> g(mu); idle.push_back(set); set = StreamSet();
    }
};
inline StreamPool& stream_pool() { static StreamPool* p = new StreamPool(); return *p; }      // (never destructed: no order of static destructors to get wrong at exit)

// The set a context holds, handed back (synchronised, then idle) when the lease ends.  A set that could not be completed is never held: the streams created before the
// failure are neither destroyed nor pooled (the next context would get null streams).
struct StreamLease {
    StreamSet set;
    StreamLease() = default; StreamLease(const StreamLease&) = delete; StreamLease& operator=(const StreamLease&) = delete;
    ~StreamLease() { stream_pool().release(set); }
    hipError_t acquire(int device) { StreamSet s; const hipError_t e = stream_pool().acquire(device, s); if (e == hipSuccess) set = s; return e; }
};

}  // namespace rtx

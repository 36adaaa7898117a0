// rtx_k_trace.hpp — the two persistent traversal kernels of the general path (closest hit, any hit).  Their stack is TraceStack<STK> (rtx_traverse.hpp); a visible
// NEE sample is added by add_visible (rtx_shade.hpp), as in phase 3 of k_bounce_bvh.  The persistent loop (refill, wave-schedule step, retire) is written out in each
// kernel on purpose: these kernels are compiled to a 64-VGPR cap, and with one lambda-taking driver the any-hit kernel compiled to 64 instead of 62 VGPRs (LDS stack) and
// to 2 spilled VGPRs (overflow stack).
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
#pragma once
#include "rtx_shade.hpp"

namespace rtx {

// RTX_OPT_TRACE_COUNTERS: a wave adds its lanes' tallies of node steps and triangle tests to two 64-bit counters (one atomic pair per wave, at its exit)
__device__ __forceinline__ void trace_count_flush(unsigned long long* cnt, uint32_t nodes, uint32_t tris) {
    unsigned long long a = nodes, b = tris;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { a += __shfl_xor(a, d); b += __shfl_xor(b, d); }
    if (lane_id() == 0) { atomicAdd(cnt, a); atomicAdd(cnt + 1, b); }
}
#ifndef RTX_TRACE_WAVES
#define RTX_TRACE_WAVES 8          // waves per SIMD the DEFAULT-schedule instantiations (SCHED >= 0) of the persistent traversal kernels are compiled for: 62 VGPRs, no spills.  (Uncapped, the
                                  // closest-hit kernel took 69 VGPRs = 7 waves once the 6-B stack entries let eight workgroups fit a CU's LDS.)  The generic instantiations (SCHED -1: experiment
                                  // knobs, work counters) stay uncapped: capped they spill
#endif
#ifndef RTX_TRACE_WAVES_CUT
#define RTX_TRACE_WAVES_CUT 8      // ... and their CUT forms (profiles/cutout_kernel_resources.md)
#endif
// closest hit for every path in this workgroup's sub-queue: reads ray_o/ray_d, writes hit
// CUT (both kernels): the scene has a cut-out triangle (sc.tri_cut != nullptr) and every geometric candidate goes through cut_accept (rtx_cutout.hpp); scenes without one launch
// the CUT = false instantiations, which are the code they always were.  No STEAL instantiation has a CUT form (RTX_OPT_WORK_STEALING is ignored while cut-outs are active).
template <int STK, bool STEAL, int SCHED, bool CUT = false>   // traversal stack: 0 = LDS column, 1 = private (scratch); STEAL: work stealing between sub-queues (refill_steal);
                                            // SCHED: the wave schedule as a compile-time constant (the default, 6), or -1 = the run-time parameter (experiment knobs)
__global__ __launch_bounds__(kBlock, (SCHED >= 0 ? (CUT ? RTX_TRACE_WAVES_CUT : RTX_TRACE_WAVES) : 1)) void k_trace_closest(DevScene sc, const SmallRecPair* __restrict__ small, DevPaths p, const uint32_t* __restrict__ queue, const uint32_t* __restrict__ qcount, uint32_t qcap, float tmin, uint32_t refill_min, uint32_t sched, uint32_t* heads,
                                                                       uint32_t nq, uint32_t merge) {           // nq sub-queues in the launch, `merge` of them per workgroup (MergedQ; 1 with STEAL and on the tiny-scene test path)
    extern __shared__ F4 lds[];
    __shared__ uint32_t s_head;
#ifdef RTX_WAVE_CLOCK
    #define RTX_WAVE_STAMP(K) do { const uint32_t w_ = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); if (tmin != kTMinCam && lane_id() == 0 && w_ < 65536u) g_wgt[2u * w_ + (K)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    RTX_WAVE_STAMP(0u);
#endif
    MergedQ M; M.init(qcount, nq, merge);
    const uint32_t n = M.n;
    if (STEAL ? all_exhausted(heads, gridDim.x) : n == 0) return;      // (work stealing: nothing left in the whole launch)
    if (threadIdx.x == 0) s_head = 0;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const bool sorted = !STEAL && p.perm != nullptr && p.oct_in != nullptr && p.out_o != nullptr;      // RTX_OPT_OCTANT_SORT: every sub-queue of this workgroup grouped by direction octant
    if (sorted) for (uint32_t t = 0; t < merge && M.q0 + t < nq; t++) sort_by_key(p.oct_in + (size_t)(M.q0 + t) * qcap, p.perm + (size_t)(M.q0 + t) * qcap, qcount[M.q0 + t], L.stack);
    const uint32_t* myq = queue + (size_t)blockIdx.x * qcap;
    if (SCHED < 0 && sc.nsmall) {                          // tiny scene, un-fused kernels (test path)
        for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
            const uint32_t pid = p.out_o ? blockIdx.x * qcap + i : myq[i];       // compact state: the queue position is the index
            const F4 ro = p.ray_o[pid], rd = p.ray_d[pid];
            float t, u, v; uint32_t prim;
            traverse_small<false>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), tmin, kTMax, t, u, v, prim, sc.nsmall);
            p.hit[pid] = {t, u, v, u2f(prim)};
        }
        return;
    }
    TraceStack<STK> stk; stk.init(L);
    RayLane R; ray_idle(R);
    bool drained = false;
    RaySource W{heads, qcount, gridDim.x, blockIdx.x, n, 0u, 0u};
    uint32_t rng = steal_seed();
    uint32_t cnt_nodes = 0, cnt_tris = 0;
    auto fetch = [&](uint32_t q, uint32_t idx) {
        if (sorted) idx = p.perm[(size_t)q * qcap + idx];
        const uint32_t pid = p.out_o ? q * qcap + idx : queue[(size_t)q * qcap + idx];
        const F4 ro = ld_stream(p.ray_o + pid), rd = ld_stream(p.ray_d + pid);
        ray_begin(R, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), tmin, kTMax, pid, true);
    };
    while (STEAL ? refill_steal<true>(R, W, drained, refill_min, rng, fetch) : refill<true>(R, &s_head, n, drained, refill_min, [&](uint32_t idx) { uint32_t q, off; M.locate(idx, q, off); fetch(q, off); })) {
        if (SCHED >= 5) spec_step<false, decltype(stk), false, CUT>(sc, L, R, stk, (uint32_t)SCHED);
        else if (sched >= 5u) spec_step<false, decltype(stk), true, CUT>(sc, L, R, stk, sched, &cnt_nodes, &cnt_tris);
        else if (sched) voted_step<false, decltype(stk), CUT>(sc, L, R, stk, sched);
        else { walk_internal<false>(sc, L, R, stk); process_leaf<false, decltype(stk), CUT>(sc, L, R, stk); }
        if (R.has && R.done) { st_stream(p.hit + R.item, F4{R.bt, R.bu, R.bv, u2f(R.bprim)}); R.has = false; }
    }
    if (SCHED < 0 && sc.trace_cnt) trace_count_flush(sc.trace_cnt, cnt_nodes, cnt_tris);      // RTX_OPT_TRACE_COUNTERS (generic instantiation only)
#ifdef RTX_WAVE_CLOCK
    RTX_WAVE_STAMP(1u);
#endif
}

// any-hit for NEE slot j: visible contributions are added to the path's radiance (a path appears at most once
// per slot, so the read-modify-write needs no atomic and the order of additions per path is fixed)
// SINK 0: the path tracer's NEE rays (visible contributions are added to the path's radiance).  SINK 1: visibility rays of the ReSTIR stages (rtx_restir_wave.hpp):
// the answer goes to occ[pay[entry]] as a byte, 1 = occluded; end points may be anywhere (last frame's samples), so the tiny-scene path tests every record.
template <int STK, bool STEAL, int SCHED, int SINK = 0, bool CUT = false>
__global__ __launch_bounds__(kBlock, (SCHED >= 0 ? (CUT ? RTX_TRACE_WAVES_CUT : RTX_TRACE_WAVES) : 1)) void k_trace_shadow(DevScene sc, const SmallRecPair* __restrict__ small, DevPaths p, const F4* __restrict__ sh_o, const F4* __restrict__ sh_d,
                                                         const F4* __restrict__ sh_c, const uint32_t* __restrict__ shcount, uint32_t qcap, uint32_t refill_min, uint32_t sched, uint32_t* heads,
                                                         uint32_t nq, uint32_t merge, const uint32_t* __restrict__ pay = nullptr, uint8_t* __restrict__ occ = nullptr) {
    extern __shared__ F4 lds[];
    __shared__ uint32_t s_head;
#ifdef RTX_WAVE_CLOCK        // tooling build: the FIRST any-hit launch after a reset (bounce 0's shadow rays, which overlap the stamped closest-hit launch of bounce 1), waves 32768 ...
    #define RTX_WAVE_STAMP_S(K) do { const uint32_t w_ = 32768u + blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); if (!SINK && lane_id() == 0 && w_ < 65536u && g_wgt[2u * w_ + (K)] == 0ull) g_wgt[2u * w_ + (K)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    RTX_WAVE_STAMP_S(0u);
#endif
    MergedQ M; M.init(shcount, nq, merge);
    const uint32_t n = M.n;
    if (STEAL ? all_exhausted(heads, gridDim.x) : n == 0) return;
    if (threadIdx.x == 0) s_head = 0;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const size_t qb = (size_t)blockIdx.x * qcap;
    auto finish = [&](size_t gi, bool occluded) {         // gi: index into the launch's shadow-ray arrays (sub-queue * qcap + entry)
        if (SINK) { occ[pay[gi]] = occluded ? 1 : 0; return; }
        if (!occluded) add_visible(p, sh_c, gi);
    };
    if (SCHED < 0 && sc.nsmall) {
        for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
            const F4 so = sh_o[qb + i], sd = sh_d[qb + i];
            float t, u, v; uint32_t prim;
            const uint32_t nrec_sh = (SINK || __builtin_amdgcn_ballot_w64(so.w < 0.0f) != 0ull) ? sc.nsmall : sc.nsmall_occ;                        // hull guard, as in k_bounce_small
            traverse_small<true>(sc, small, L, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z), SINK ? so.w : fabsf(so.w), sd.w, t, u, v, prim, nrec_sh);   // the short list: NEE segments only
            finish(qb + i, prim != kMissPrim);
        }
        return;
    }
    TraceStack<STK> stk; stk.init(L);
    RayLane R; ray_idle(R);
    bool drained = false;
    RaySource W{heads, shcount, gridDim.x, blockIdx.x, n, 0u, 0u};
    uint32_t rng = steal_seed();
    uint32_t cnt_nodes = 0, cnt_tris = 0;
    auto fetch = [&](uint32_t q, uint32_t idx) {
        const uint32_t gi = q * qcap + idx;                               // (< 2^32: the batch cap)
        const F4 so = sh_o[gi], sd = sh_d[gi];
        ray_begin(R, mk3(so.x, so.y, so.z), mk3(sd.x, sd.y, sd.z), so.w, sd.w, gi, false, !CUT && sc.occluder_cache != 0u, sc.any_order);      // (RTX_OPT_OCCLUDER_CACHE is ignored while cut-outs are active)
    };
    while (STEAL ? refill_steal<false>(R, W, drained, refill_min, rng, fetch) : refill<false>(R, &s_head, n, drained, refill_min, [&](uint32_t idx) { uint32_t q, off; M.locate(idx, q, off); fetch(q, off); })) {
        if (SCHED >= 5) spec_step<true, decltype(stk), false, CUT>(sc, L, R, stk, (uint32_t)SCHED);
        else if (sched >= 5u) spec_step<true, decltype(stk), true, CUT>(sc, L, R, stk, sched, &cnt_nodes, &cnt_tris);
        else if (sched) voted_step<true, decltype(stk), CUT>(sc, L, R, stk, sched);
        else { walk_internal<true>(sc, L, R, stk); process_leaf<true, decltype(stk), CUT>(sc, L, R, stk); }
        if (R.has && R.done) { finish(R.item, R.bprim != kMissPrim); R.has = false; }
    }
    if (SCHED < 0 && sc.trace_cnt) trace_count_flush(sc.trace_cnt + 2, cnt_nodes, cnt_tris);
#ifdef RTX_WAVE_CLOCK
    RTX_WAVE_STAMP_S(1u);
#endif
}

}  // namespace rtx

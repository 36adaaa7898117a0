// rtx_bounce_small_parts.hpp — what the three bodies of k_bounce_small (rtx_k_bounce_small.hpp: bounce 0, block schedule; rtx_k_bounce_wave.hpp: wave schedule) have in common,
// each defined once.  Every part is inlined and holds exactly the statements a body would otherwise spell out; profiles/bounce_parts_kernel_resources.md compares the ten
// instantiations with their written-out form row by row (occupancy, LDS, barriers and the tables in LDS are kept; the few columns that moved are listed there).
// Uses the PF_* section-profile macros that rtx_kernels.hip defines before it includes the kernel headers (a part that counts takes the body's `pf`).
#pragma once
#include "rtx_shade.hpp"

namespace rtx {

// (round 5) the light list (<= kSmallLights records + CDF) and the material table (<= kSmallMats records) of a tiny scene in LDS: with five workgroups per CU the dependent global
// reads of NEE's CDF search, the light record and the material record are not hidden by other waves (k_shade gained 17 % from the same on the street scene).  A longer table
// stays in global memory (lights / cdf = nullptr: nee_sample then reads the scene's).  The caller's next workgroup barrier makes the tables visible.
// (the shade records and normal matrices as well, 4.3 KB more, cost the fifth workgroup per CU: 18.09 vs 18.03 ms without any table on the same box — not kept)
struct SmallTables { const MatGPU* mats; const LightGPU* lights; const float* cdf; };
// STAGE_SMALL_TABLES(T, sc): declares the tables in the body's own LDS, fills them and defines `const SmallTables T`.  A macro in the style of RS_STAGE_SCENE, not a function
// with the arrays inside: a function's arrays are ONE set for all ten instantiations, and the compiler then spills differently (profiles/bounce_parts_kernel_resources.md).
#ifndef RTX_NO_SMALL_LDS_TABLES
#define STAGE_SMALL_TABLES(T, sc) \
    __shared__ F4 s_lt[kSmallLights * 5]; __shared__ float s_ltcdf[kSmallLights]; __shared__ F4 s_mt[kSmallMats * 10]; \
    const bool lt_lds = sc.nlights && sc.nlights <= kSmallLights, mt_lds = sc.nmat && sc.nmat <= kSmallMats; \
    if (lt_lds) { for (uint32_t i = threadIdx.x; i < sc.nlights * 5u; i += kBlock) s_lt[i] = ((const F4*)sc.lights)[i]; if (threadIdx.x < sc.nlights) s_ltcdf[threadIdx.x] = sc.cdf[threadIdx.x]; } \
    if (mt_lds) for (uint32_t i = threadIdx.x; i < sc.nmat * 10u; i += kBlock) s_mt[i] = ((const F4*)sc.mats)[i]; \
    const SmallTables T = {mt_lds ? (const MatGPU*)s_mt : sc.mats, lt_lds ? (const LightGPU*)s_lt : nullptr, lt_lds ? s_ltcdf : nullptr}
#else
#define STAGE_SMALL_TABLES(T, sc) const SmallTables T = {sc.mats, nullptr, nullptr}
#endif

// hit -> shading decision of one item whose ray hit `prim`: true when the surface is to be shaded (NEE, continuation); an emissive surface adds its radiance and ends the path
// HAVE_HIT (k_bounce_small): 2 = `sf` already holds the pixel's shared surface; != 0 = bounce 0, nothing has written the path's radiance slot yet (an out-of-range material
// leaves it black)
template <int HAVE_HIT>
__device__ __forceinline__ bool hit_to_shading(const DevScene& sc, const DevPaths& p, const MatGPU* mats, const PathState& S, Surf& sf, float t, float u, float v, uint32_t prim, uint32_t bounce, uint32_t nee) {
    if (HAVE_HIT != 2) sf = surface(sc, S.o, S.d, t, u, v, prim);
    if (sf.mat < sc.nmat) {
        const MatGPU& m = mats[sf.mat];
        if (m.Ke_len > 0.0f) add_emissive(sc, p, S, sf, m, bounce, nee, HAVE_HIT != 0);
        else return true;
    } else if (HAVE_HIT) p.rad[S.pid] = {0.0f, 0.0f, 0.0f, 0.0f};
    return false;
}

// triangle records a block of shadow rays tests: the hull-face shortcut (sc.nsmall_occ) only if no ray of this wave starts near a hull plane (flag in the sign of tmin, TriShade::guard_tau)
__device__ __forceinline__ uint32_t shadow_records(const DevScene& sc, bool mine, float tmin_flag) {
    return __builtin_amdgcn_ballot_w64(mine && tmin_flag < 0.0f) != 0ull ? sc.nsmall : sc.nsmall_occ;
}

// PATH STATE BY QUEUE POSITION (COMPACT, RTX_OPT_COMPACT_STATE; DevPaths::out_o != nullptr is the flag, as for the separate kernels).  ray_o / ray_d / thr hold TWO sets of
// G * qcap entries each, set 1 the same distance behind set 0 in all three streams (state_set_stride).  Bounce b reads the state of queue entry i of sub-queue q at
// (b & 1) * stride + q * qcap + i and writes a survivor's state into the OTHER set at the slot it takes in the next queue: a wave's state accesses are one contiguous run however
// many paths died before, and the extension trace fetches its rays without reading the queue first.  The queues still carry the path id, read where it is needed: the
// radiance additions (rad stays by path id) and the next queue's entry.  Bounce 0 is a launch of its own: with the hit buffer as input (HAVE_HIT 1) it reads set 0 by PATH ID,
// where k_raygen_trace_small wrote it, and writes set 1 by position.  !COMPACT: by path id, updated in place.
__device__ __forceinline__ uint32_t state_set_stride(const DevPaths& p) { return (uint32_t)(p.out_o - p.ray_o); }
// first entry of sub-queue base `qb` in the set that bounce `bounce` reads (state_in) / writes (state_out)
__device__ __forceinline__ uint32_t state_in(uint32_t qb, uint32_t stride, uint32_t bounce) { return qb + ((bounce & 1u) ? stride : 0u); }
__device__ __forceinline__ uint32_t state_out(uint32_t qb, uint32_t stride, uint32_t bounce) { return qb + ((bounce & 1u) ? 0u : stride); }

// continuation of one item (go = it was shaded and this is not the last bounce): BSDF sample, throughput, Russian roulette; a surviving path stores its state and takes a slot of
// the sub-queue's next queue (s_cnt0 = its length so far).  Every lane of the workgroup's waves goes through the compaction.
// COMPACT: the state goes to out0 + slot (out0 = state_out of this bounce), else to the path's own record.
template <bool COMPACT>
__device__ __forceinline__ void continue_path(const MatGPU& m, const DevFrame& f, const DevPaths& p, uint32_t bounce, bool go, PathState& S, f3 pos, f3 normal, f3 outgoing, float eta_p,
                                              uint32_t* s_cnt0, uint32_t* mynext, uint32_t out0, Prof* pf) {
    bool alive = false;
    f3 smp; float P;                                              // no initialiser: read under `alive` only, and bsdf_continue assigns both before it returns true
    if (go) { PF_COUNT(9); alive = bsdf_continue(m, f, bounce, S, normal, outgoing, smp, P, eta_p); }
    if (!COMPACT && alive) { PF_COUNT(10); store_path(p, S, pos, smp, P); }
    const uint32_t slot = block_push(alive, s_cnt0);
    if (COMPACT && alive) { PF_COUNT(10); store_path_at(p.ray_o, p.ray_d, p.thr, out0 + slot, S, pos, smp, P); }
    if (alive) mynext[slot] = S.pid;
}

// end of bounce `bounce` of sub-queue `qid`: publish its counters (s_cnt[0] = entries of the next queue, the return value; s_cnt[1 + j] = shadow rays of NEE slot j) and clear them —
// and, CURSOR, the input cursor s_in of the wave schedule — for the next bounce.  Three workgroup barriers: what the bounce wrote (path state, radiance, next queue) becomes visible to the
// workgroup; the counters are read before they are cleared; they are cleared before the next bounce counts.
template <bool CURSOR>
__device__ __forceinline__ uint32_t end_bounce(uint32_t* s_cnt, uint32_t* s_in, uint32_t* qrows, uint32_t* srows, uint32_t bounce, uint32_t G, uint32_t qid, uint32_t nee) {
    const uint32_t nee1 = nee ? nee : 1u;
    __syncthreads();
    const uint32_t n = s_cnt[0];
    if (threadIdx.x == 0) qrows[(size_t)(bounce + 1u) * G + qid] = n;
    if (threadIdx.x >= 1 && threadIdx.x <= nee) srows[((size_t)bounce * nee1 + (threadIdx.x - 1)) * G + qid] = s_cnt[threadIdx.x];
    __syncthreads();
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    if (CURSOR && threadIdx.x == 0) *s_in = 0;
    __syncthreads();
    return n;
}

// tooling build (-DRTX_WAVE_CLOCK, tools/wave_timeline.py cornell): wave start (k = 0) / end (k = 1) stamps of the launch of bounces >= 1
__device__ __forceinline__ void wave_stamp(uint32_t k) {
#ifdef RTX_WAVE_CLOCK
    const uint32_t w = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
    if (lane_id() == 0 && w < 65536u) g_wgt[2u * w + k] = __builtin_amdgcn_s_memrealtime();
#endif
}

}  // namespace rtx

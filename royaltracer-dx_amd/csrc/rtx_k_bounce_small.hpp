// rtx_k_bounce_small.hpp — the fused bounce kernel of tiny scenes
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
// Uses the PF_* section-profile macros that rtx_kernels.hip defines before it includes this file.
#pragma once
#include "rtx_shade.hpp"
#include "rtx_k_bounce_wave.hpp"   // the body of RING == 2

namespace rtx {

// Fused bounce kernel for tiny scenes (sc.nsmall != 0): trace the extension ray, shade, trace the NEE shadow
// rays and add their contributions, sample the BSDF, compact — all in one pass over the workgroup's sub-queue.
// Nothing but the 48-B path state and the queue index moves through HBM; hit records and shadow-ray entries
// stay in registers.  Radiance additions happen in the oracle's order (emissive, then NEE slot 0, 1, ...).
// LAMBERT: RTX_FLAG_LAMBERT_ONLY is a launch constant, so it is a template parameter too: the Lambert-only instantiation carries no GGX code
// (fewer live registers, fewer SGPR spills through v_writelane / v_readlane in the loop).
// HAVE_HIT: 0 = bounces >= 1 (the kernel traces its extension rays); bounce 0: 1 = path state and hit record come from k_raygen_trace_small, 2 = RTX_OPT_SHARED_PRIMARY: the
// path starts from its pixel's shared record (k_primary_surface) and derives sample, slot and seeds from its id (PrimIn) — no surface() here, and nothing per path read but the queue word
// RING (bounces >= 1, RTX_OPT_BOUNCE_VARIANT): 1 = workgroup-wide LDS hit ring between trace and shading (variant 0); 0 = trace and shade the same 256 entries (variant 1);
// 2 = wave-private rings, no barrier inside a bounce (variant 2): its body is bounce_small_wave(), rtx_k_bounce_wave.hpp
template <int WAVES, int HAVE_HIT, bool LAMBERT, int RING>
__global__ __launch_bounds__(kBlock, WAVES) void k_bounce_small(DevScene sc, const SmallRecPair* __restrict__ small, DevFrame f_in, DevPaths p,
                                                         uint32_t bounce_first, uint32_t bounce_end,
                                                         uint32_t* __restrict__ queue_a, uint32_t* __restrict__ queue_b /* bounce b reads (b & 1 ? b : a), writes the other */,
                                                         uint32_t* __restrict__ qrows /* [bounce][gridDim.x] sub-queue lengths entering each bounce */,
                                                         uint32_t* __restrict__ srows /* [bounce][nee][gridDim.x]: shadow rays traced (statistics) */,
                                                         const uint32_t* __restrict__ order /* workgroup -> sub-queue, longest first (k_order_queues); may be null */,
                                                         PrimIn pin /* HAVE_HIT 2: the per-pixel records of k_primary_surface and how to find a path's (read by that instantiation only) */) {
    // BOUNCE RANGE: sub-queues are workgroup-private, so bounce b + 1 of sub-queue q depends on bounce b of the SAME sub-queue only.  One
    // launch therefore runs the bounces [bounce_first, bounce_end) of its sub-queue back to back, with a workgroup barrier in between
    // (workgroup-scope release / acquire: the path state and queue entries a bounce writes are read by the same workgroup).  A frame has
    // two fused launches (bounce 0, which reads the primary hits, and bounces 1 .. max_bounces - 1) instead of eight, and no drain /
    // ramp-up between the bounces; the sparsely populated late bounces cost a few loop trips instead of a launch each.
    if constexpr (RING == 2) { bounce_small_wave<LAMBERT>(sc, small, f_in, p, bounce_first, bounce_end, queue_a, queue_b, qrows, srows, order); return; }
    else {
    extern __shared__ F4 lds[];
    __shared__ uint32_t s_cnt[1 + kMaxNee];
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);           // bit 0 of the flags known at compile time
    const uint32_t qid = order ? order[blockIdx.x] : blockIdx.x;      // the sub-queue this workgroup owns (input and output)
#ifdef RTX_WAVE_CLOCK        // tooling build: wave start / end stamps of the launch of bounces >= 1 (tools/wave_timeline.py cornell)
    #define RTX_WAVE_STAMP_B(K) do { const uint32_t w_ = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6); if (!HAVE_HIT && lane_id() == 0 && w_ < 65536u) g_wgt[2u * w_ + (K)] = __builtin_amdgcn_s_memrealtime(); } while (0)
    RTX_WAVE_STAMP_B(0u);
#endif
    // NEE shadow rays of the workgroup's 256 current items are compacted through LDS, so that the shadow traversal runs on
    // ceil(rays / 64) full waves instead of on every wave at ~2/3 occupancy (only ~65 % of the items get a shadow ray)
    __shared__ F4 s_sho[kBlock], s_shd[kBlock];
    __shared__ uint32_t s_shn[2];                          // ray count, double-buffered by iteration parity
    __shared__ uint8_t s_occ[kBlock];
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 2) s_shn[threadIdx.x] = 0;
    // (round 5) the light list (<= 32 records + CDF) and the material table (<= 16 records) of a tiny scene in LDS: with five workgroups per CU the dependent global reads of NEE's
    // CDF search, the light record and the material record are not hidden by other waves (k_shade gained 17 % from the same on the street scene)
#ifndef RTX_NO_SMALL_LDS_TABLES
    constexpr uint32_t kSmallLights = 32, kSmallMats = 16;
    __shared__ F4 s_lt[kSmallLights * 5]; __shared__ float s_ltcdf[kSmallLights]; __shared__ F4 s_mt[kSmallMats * 10];
    const bool lt_lds = sc.nlights && sc.nlights <= kSmallLights, mt_lds = sc.nmat && sc.nmat <= kSmallMats;
    if (lt_lds) { for (uint32_t i = threadIdx.x; i < sc.nlights * 5u; i += kBlock) s_lt[i] = ((const F4*)sc.lights)[i]; if (threadIdx.x < sc.nlights) s_ltcdf[threadIdx.x] = sc.cdf[threadIdx.x]; }
    if (mt_lds) for (uint32_t i = threadIdx.x; i < sc.nmat * 10u; i += kBlock) s_mt[i] = ((const F4*)sc.mats)[i];
    const MatGPU* mats = mt_lds ? (const MatGPU*)s_mt : sc.mats;
    const LightGPU* lds_lights = lt_lds ? (const LightGPU*)s_lt : nullptr; const float* lds_cdf = lt_lds ? s_ltcdf : nullptr;
    // (the shade records and normal matrices as well, 4.3 KB more, cost the fifth workgroup per CU: 18.09 vs 18.03 ms without any table on the same box — not kept)
#else
    const MatGPU* mats = sc.mats; const LightGPU* lds_lights = nullptr; const float* lds_cdf = nullptr;
#endif
    const uint32_t G = gridDim.x;
    uint32_t n = qrows[(size_t)bounce_first * G + qid];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const uint32_t nee1 = nee ? nee : 1u;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const size_t qb = (size_t)qid * f.qcap;
    uint32_t par = 0;
    // HIT RING (bounces >= 1).  20-25 % of the extension rays of a bounce leave the open front of the box or end on the light, and their lanes used to idle
    // through surface reconstruction, NEE and BSDF sampling — over half of the kernel's instructions (46-47 of 64 lanes active per VALU instruction,
    // profiles/r02_pmc_cornell.md).  Tracing and shading are therefore decoupled inside the workgroup: the trace phase takes 256 queue entries at a time
    // and pushes only the HITS (path slot + hit record, 20 B) into an LDS ring (ballot + one LDS atomic per wave); whenever the ring holds a full 256 (or
    // the input is exhausted) the shading phase runs on ring entries, i.e. on full waves.  A miss costs nothing beyond its trace.  The price: the path state
    // is read twice (origin / direction for the trace, all 48 B for the shading), which a VALU-bound kernel at 2.4 of 8 TB/s does not notice.
    // All four waves walk through the same phases (every decision is read from LDS after a barrier), so there is no producer / consumer protocol.
    constexpr uint32_t kRing = 512u;                       // < 256 waiting + <= 256 pushed by one trace pass
    __shared__ uint32_t s_rpid[(HAVE_HIT || !RING) ? 1 : kRing];
    __shared__ F4 s_rhit[(HAVE_HIT || !RING) ? 1 : kRing];
    // Ring counters.  s_ring[0] = entries consumed (written by thread 0 between two barriers).  Entries PRODUCED are counted per trace pass in one of three
    // rotating LDS words (pass k pushes into s_rc[k % 3]) and summed in a register (`prod`) after the barrier that ends the pass: the loop condition below then
    // depends on registers and on s_ring[0] only, never on a word another wave may be pushing into.  (With ONE produced-counter read in the condition, a wave
    // that evaluated it late could see a push of the current pass, leave the loop and strand the others at the barrier — a formal race)  A word is
    // cleared by thread 0 after the barrier of pass k + 1 and next pushed into in pass k + 3; it was last read before that barrier.
    __shared__ uint32_t s_ring[1], s_rc[3];
    PF_BEGIN;
    for (uint32_t bounce = bounce_first; bounce < bounce_end; bounce++) {
    const bool last = (bounce + 1u == f.max_bounces);
    const float tmin = bounce_tmin(bounce);
    const uint32_t sbounce = HAVE_HIT == 2 ? 0u : bounce;     // what the shading sees: that instantiation is launched for bounce 0 only, so its MIS and Russian-roulette branches fold away
    const uint32_t* myq = ((bounce & 1u) ? queue_b : queue_a) + qb;
    uint32_t* mynext = ((bounce & 1u) ? queue_a : queue_b) + qb;
    if (!HAVE_HIT && RING) { if (threadIdx.x < 3) s_rc[threadIdx.x] = 0; if (threadIdx.x == 3) s_ring[0] = 0; __syncthreads(); }
    uint32_t next_in = 0;                                   // trace phase: next input entry (uniform)
    uint32_t prod = 0, rk = 0;                              // hits pushed by the completed trace passes of this bounce; pass number mod 3 (both uniform)
    for (uint32_t base = 0; (HAVE_HIT || !RING) ? base < n : true; base += kBlock) {     // one trip per 256 queue entries; with the ring: until input and ring are empty
        PathState S; S.pid = 0; S.o = mk3(0, 0, 0); S.d = mk3(0, 0, 1); S.thr = mk3(0, 0, 0); S.prev_pdf = 1.0f; S.s0 = S.s1 = 0;
        float t = 0.0f, u = 0.0f, v = 0.0f; uint32_t prim = kMissPrim;
        bool active;
        PF_MARK(0);
        Surf sf; sf.mat = 0; sf.normal = mk3(0, 0, 1); sf.pos = mk3(0, 0, 0);
        if (HAVE_HIT == 2) {                              // bounce 0 from the shared record: every queue entry is a hit, its surface is the pixel's
            const uint32_t i = base + threadIdx.x;
            active = i < n;
            if (active) {
                S.pid = myq[i];
                // pid = sl * f.npl + v: the batch's sample, the (virtual) slot; the division is exact for every pid < 2^31 (PrimIn)
                const uint32_t sl = __umulhi(S.pid, pin.div_mul) >> pin.div_shift, v = S.pid - sl * f.npl;
                const uint32_t pl = f.list ? f.list[v >> 8] * (uint32_t)kBlock + (v & 255u) : v;       // real_slot: a pass of rtx_render_adaptive
                const F4 r0 = pin.rec[pl], r1 = pin.rec[(size_t)pin.npl + pl], r2 = pin.rec[(size_t)2 * pin.npl + pl], ro = pin.rec[(size_t)3 * pin.npl];
                seed_sample(f2u(r2.w), f2u(r1.w), f.sample_first + sl, f.frame_seed, S.s0, S.s1);     // = seed_init(x, y, sample, frame_seed): the record carries the pixel's terms
                S.o = mk3(ro.x, ro.y, ro.z); S.d = mk3(r0.x, r0.y, r0.z); S.thr = mk3(1.0f, 1.0f, 1.0f); S.prev_pdf = 1.0f;
                sf.pos = mk3(r1.x, r1.y, r1.z); sf.normal = mk3(r2.x, r2.y, r2.z); sf.mat = f2u(r0.w) & 0x7FFFFFFFu; sf.near_hull = (f2u(r0.w) >> 31) != 0u;
                prim = 0u;                                                     // (any id but kMissPrim)
            }
        } else if (HAVE_HIT) {                            // bounce 0: the primary hit comes from k_raygen_trace_small; every queue entry is a hit
            const uint32_t i = base + threadIdx.x;
            active = i < n;
            if (active) { S = load_path(p, myq[i]); const F4 h = p.hit[S.pid]; t = h.x; u = h.y; v = h.z; prim = f2u(h.w); }
        } else if (!RING) {                               // RTX_OPT_BOUNCE_VARIANT = 1: trace and shade the same 256 entries (lanes whose ray missed idle through the shading)
            const uint32_t i = base + threadIdx.x;
            active = i < n;
            if (active) S = load_path(p, myq[i]);
            traverse_small<false>(sc, small, L, S.o, S.d, tmin, active ? kTMax : 0.0f, t, u, v, prim, sc.nsmall, ~0ull, pf, 1);   // inactive lanes: empty interval
        } else {
            // ---- trace phase: fill the ring until it holds a full workgroup of hits (or the input runs out) ----
            while (next_in < n && prod - s_ring[0] < kBlock) {                // uniform: `prod` is a register, s_ring[0] was written before the last barrier
                const uint32_t i = next_in + threadIdx.x;
                const bool act = i < n;
                uint32_t pid = 0; f3 ro = mk3(0, 0, 0), rd = mk3(0, 0, 1);
                if (act) { pid = myq[i]; const F4 a = p.ray_o[pid], b = p.ray_d[pid]; ro = mk3(a.x, a.y, a.z); rd = mk3(b.x, b.y, b.z); }
                float ht, hu, hv; uint32_t hp;
                traverse_small<false>(sc, small, L, ro, rd, tmin, act ? kTMax : 0.0f, ht, hu, hv, hp, sc.nsmall, ~0ull, pf, 1);   // inactive lanes: empty interval
                const bool hit = act && hp != kMissPrim;
                const uint32_t slot = prod + block_push(hit, &s_rc[rk]);
                if (hit) { s_rpid[slot & (kRing - 1u)] = pid; s_rhit[slot & (kRing - 1u)] = {ht, hu, hv, u2f(hp)}; }
                next_in += kBlock;
                __syncthreads();
                prod += s_rc[rk];                                               // this pass's pushes are complete; the word stays untouched for two more passes
                if (threadIdx.x == 0) s_rc[rk == 0u ? 2u : rk - 1u] = 0;        // the word of the PREVIOUS pass: every wave read it before the barrier above; next used two passes from now
                rk = rk == 2u ? 0u : rk + 1u;
            }
            const uint32_t head = s_ring[0], avail = prod - head;
            if (avail == 0u) break;                                             // input exhausted and ring drained: this bounce is done (uniform)
            const uint32_t take = avail < (uint32_t)kBlock ? avail : (uint32_t)kBlock;
            active = threadIdx.x < take;
            if (active) {
                const uint32_t e = (head + threadIdx.x) & (kRing - 1u);
                S = load_path(p, s_rpid[e]);
                const F4 h = s_rhit[e]; t = h.x; u = h.y; v = h.z; prim = f2u(h.w);
            }
            __syncthreads();                                                    // every lane has read its entry before the slots are released
            if (threadIdx.x == 0) s_ring[0] = head + take;
        }
        PF_MARK(2);
        bool shading = false;
        if (active && prim != kMissPrim) {
            PF_COUNT(3);
            if (HAVE_HIT != 2) sf = surface(sc, S.o, S.d, t, u, v, prim);
            if (sf.mat < sc.nmat) {
                const MatGPU& m = mats[sf.mat];
                if (m.Ke_len > 0.0f) add_emissive(sc, p, S, sf, m, sbounce, nee, HAVE_HIT != 0);
                else shading = true;
            } else if (HAVE_HIT) p.rad[S.pid] = {0.0f, 0.0f, 0.0f, 0.0f};
        }
        const f3 outgoing = -S.d, pos = sf.pos;
        const MatGPU* mp = mats + (shading ? sf.mat : 0u);
        f3 normal = sf.normal;
        const float eta_p = LAMBERT ? 0.0f : transmission_eta(*mp, f.flags, outgoing, normal);
        // bounce 0 (HAVE_HIT): nothing has written this path's radiance slot yet: it starts from zero here and is always stored
        bool loaded = HAVE_HIT && shading; F4 radv = {0, 0, 0, 0};
        PF_MARK(3);
        for (uint32_t j = 0; j < nee; j++) {
            bool push = false;
            F4 so = {0, 0, 0, 0}, sd = {0, 0, 1, 0}; f3 con = mk3(0, 0, 0);
            if (shading) { PF_COUNT(4); push = nee_sample(sc, *mp, f.flags, nee, S, pos, normal, outgoing, so, sd, con, sf.near_hull, eta_p, nullptr, lds_cdf, lds_lights); }
            PF_MARK(4);
            const uint32_t slot = block_push(push, &s_shn[par]);
            if (push) { s_sho[slot] = so; s_shd[slot] = sd; }
            __syncthreads();
            PF_MARK(5);
            const uint32_t ns = s_shn[par];
            if ((threadIdx.x & ~63u) < ns) {                                   // wave-uniform: this wave has rays to trace
                const bool mine = threadIdx.x < ns;
                const F4 ro = mine ? s_sho[threadIdx.x] : F4{0, 0, 0, 0}, rd = mine ? s_shd[threadIdx.x] : F4{0, 0, 1, 0};
                float st_, su_, sv_; uint32_t sprim;
                // hull-face shortcut only if no ray of this wave starts near a hull plane (flag in the sign of tmin, TriShade::guard_tau)
                const uint32_t nrec_sh = __builtin_amdgcn_ballot_w64(mine && ro.w < 0.0f) != 0ull ? sc.nsmall : sc.nsmall_occ;
                traverse_small<true>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), fabsf(ro.w), mine ? rd.w : 0.0f, st_, su_, sv_, sprim, nrec_sh, ~0ull, pf, 6);
                if (mine) s_occ[threadIdx.x] = sprim != kMissPrim ? 1 : 0;
            }
            PF_MARK(7);
            if (threadIdx.x == 0) { s_shn[par ^ 1u] = 0; s_cnt[1 + j] += ns; }
            __syncthreads();
            PF_MARK(8);
            if (push && !s_occ[slot]) {
                if (!loaded) { radv = p.rad[S.pid]; loaded = true; }
                radv.x = radv.x + con.x; radv.y = radv.y + con.y; radv.z = radv.z + con.z;
            }
            par ^= 1u;
        }
        if (loaded) p.rad[S.pid] = radv;
        bool alive = false;
        f3 smp = mk3(0, 0, 1); float P = 0.0f;
        if (shading && !last) { PF_COUNT(9); alive = bsdf_continue(*mp, f, sbounce, S, normal, outgoing, smp, P, eta_p); }
        if (alive) { PF_COUNT(10); store_path(p, S, pos, smp, P); }
        const uint32_t slot = block_push(alive, &s_cnt[0]);
        if (alive) mynext[slot] = S.pid;
        PF_MARK(9);
        if (!HAVE_HIT && RING) __syncthreads();             // the released ring slots (s_ring[0]) are visible to the next trip's trace phase
    }
    // end of this bounce of the sub-queue: publish its counters; what it wrote (path state, next queue) becomes visible to the workgroup
    __syncthreads();
    n = s_cnt[0];
    if (threadIdx.x == 0) qrows[(size_t)(bounce + 1u) * G + qid] = n;
    if (threadIdx.x >= 1 && threadIdx.x <= nee) srows[((size_t)bounce * nee1 + (threadIdx.x - 1)) * G + qid] = s_cnt[threadIdx.x];
    __syncthreads();
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    }
    PF_FLUSH;
#ifdef RTX_WAVE_CLOCK
    RTX_WAVE_STAMP_B(1u);
#endif
    }
}

}  // namespace rtx

// rtx_k_bounce_small.hpp — the fused bounce kernel of tiny scenes: k_bounce_small, its bounce-0 body and its block-scheduled body (the wave-scheduled one: rtx_k_bounce_wave.hpp)
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
// Uses the PF_* section-profile macros that rtx_kernels.hip defines before it includes this file.
#pragma once
#include "rtx_bounce_small_parts.hpp"
#include "rtx_k_bounce_wave.hpp"

namespace rtx {

// ---- the block-wide shadow phase ----
// NEE shadow rays of the workgroup's 256 current items are compacted through LDS, so that the shadow traversal runs on
// ceil(rays / 64) full waves instead of on every wave at ~2/3 occupancy (only ~65 % of the items get a shadow ray)
struct ShadowLds { F4* o; F4* d; uint32_t* n /* ray count, double-buffered by iteration parity */; uint8_t* occ; };
__device__ __forceinline__ ShadowLds block_shadow_lds() {          // (before the body's first barrier)
    __shared__ F4 s_sho[kBlock], s_shd[kBlock];
    __shared__ uint32_t s_shn[2];
    __shared__ uint8_t s_occ[kBlock];
    if (threadIdx.x < 2) s_shn[threadIdx.x] = 0;
    return {s_sho, s_shd, s_shn, s_occ};
}
// one NEE slot of the workgroup's 256 items: the lanes with push set hand in their ray (so, sd: nee_sample), full waves trace the compacted rays; true = this lane's ray is
// unoccluded.  Two workgroup barriers; `par` flips.  s_cnt_j: the bounce's shadow-ray count of this slot (statistics).
__device__ __forceinline__ bool block_shadow(const DevScene& sc, const SmallRecPair* small, const TraceLds& L, const ShadowLds& sh, uint32_t& par, bool push, const F4& so, const F4& sd, uint32_t* s_cnt_j, Prof* pf) {
    const uint32_t slot = block_push(push, &sh.n[par]);
    if (push) { sh.o[slot] = so; sh.d[slot] = sd; }
    __syncthreads();
    PF_MARK(5);
    const uint32_t ns = sh.n[par];
    if ((threadIdx.x & ~63u) < ns) {                                   // wave-uniform: this wave has rays to trace
        const bool mine = threadIdx.x < ns;
        F4 ro = unspecified4(), rd = unspecified4();            // a lane beyond the rays: any ray, with an empty interval (its candidates are cleared) and no say in the record count
        if (mine) { ro = sh.o[threadIdx.x]; rd = sh.d[threadIdx.x]; }
        float st_, su_, sv_; uint32_t sprim;
        traverse_small<true, false, true>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), fabsf(ro.w), mine ? rd.w : 0.0f, st_, su_, sv_, sprim, shadow_records(sc, mine, ro.w), ~0ull, pf, 6);
        if (mine) sh.occ[threadIdx.x] = sprim != kMissPrim ? 1 : 0;
    }
    PF_MARK(7);
    if (threadIdx.x == 0) { sh.n[par ^ 1u] = 0; *s_cnt_j += ns; }
    __syncthreads();
    PF_MARK(8);
    const bool visible = push && !sh.occ[slot];
    par ^= 1u;
    return visible;
}

// ---- the shading step of the two block-scheduled bodies ----
// One item per lane (active = the lane has one; prim = what its ray hit): shade, trace the NEE shadow rays (block_shadow) and add their contributions, sample the BSDF, compact.
// Radiance additions happen in the oracle's order (emissive, then NEE slot 0, 1, ...).  Every lane of the workgroup goes through the barriers and compactions.
// HAVE_HIT != 0 (bounce 0): nothing has written this path's radiance slot yet: it starts from zero here and is always stored
// (T, sh and sf by value, S by reference: of the shapes tried, the one at which no instantiation spills more SGPRs than with the step written out — profiles/bounce_parts_kernel_resources.md)
// COMPACT / out0: where a survivor's state goes (continue_path)
template <int HAVE_HIT, bool LAMBERT, bool COMPACT>
__device__ __forceinline__ void shade_block(const DevScene& sc, const SmallRecPair* small, const TraceLds& L, const DevFrame& f, const DevPaths& p, SmallTables T, ShadowLds sh, uint32_t& par,
                                            PathState& S, Surf sf, float t, float u, float v, uint32_t prim, bool active, uint32_t bounce, uint32_t nee, bool last, uint32_t* s_cnt, uint32_t* mynext, uint32_t out0, Prof* pf) {
    bool shading = false;
    if (active && prim != kMissPrim) { PF_COUNT(3); shading = hit_to_shading<HAVE_HIT>(sc, p, T.mats, S, sf, t, u, v, prim, bounce, nee); }
    const f3 outgoing = -S.d, pos = sf.pos;
    const MatGPU* mp = T.mats + (shading ? sf.mat : 0u);
    f3 normal = sf.normal;
    const float eta_p = LAMBERT ? 0.0f : transmission_eta(*mp, f.flags, outgoing, normal);
    bool loaded = HAVE_HIT && shading; F4 radv = {0, 0, 0, 0};
    PF_MARK(3);
    for (uint32_t j = 0; j < nee; j++) {
        bool push = false;
        F4 so, sd; f3 con;                                         // no initialiser: every read is under `push` (block_shadow returns push && ...), and nee_sample assigns all three before it returns true
        if (shading) { PF_COUNT(4); push = nee_sample(sc, *mp, f.flags, nee, S, pos, normal, outgoing, so, sd, con, sf.near_hull, eta_p, nullptr, T.cdf, T.lights); }
        PF_MARK(4);
        if (block_shadow(sc, small, L, sh, par, push, so, sd, &s_cnt[1 + j], pf)) {
            if (!loaded) { radv = p.rad[S.pid]; loaded = true; }
            radv.x = radv.x + con.x; radv.y = radv.y + con.y; radv.z = radv.z + con.z;
        }
    }
    if (loaded) p.rad[S.pid] = radv;
    continue_path<COMPACT>(*mp, f, p, bounce, shading && !last, S, pos, normal, outgoing, eta_p, &s_cnt[0], mynext, out0, pf);
    PF_MARK(9);
}

// ---- bounce 0 ----
// Every queue entry is a primary hit; there is no extension trace.  HAVE_HIT: 1 = path state and hit record come from k_raygen_trace_small; 2 = RTX_OPT_SHARED_PRIMARY: the
// path starts from its pixel's shared record (k_primary_surface) and derives sample, slot and seeds from its id (PrimIn) — no surface() here, and nothing per path read but the queue word
// COMPACT (rtx_bounce_small_parts.hpp): the survivors' state is written by queue position into set 1; the input (HAVE_HIT 1) is read by path id from set 0 either way
template <int HAVE_HIT, bool LAMBERT, bool COMPACT>
__device__ __forceinline__ void bounce_small_first(const DevScene& sc, const SmallRecPair* small, const DevFrame& f_in, const DevPaths& p, uint32_t bounce_first, uint32_t bounce_end,
                                                   uint32_t* queue_a, uint32_t* queue_b, uint32_t* qrows, uint32_t* srows, const uint32_t* order, const PrimIn& pin) {
    extern __shared__ F4 lds[];
    __shared__ uint32_t s_cnt[1 + kMaxNee];
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);           // bit 0 of the flags known at compile time
    const uint32_t qid = order ? order[blockIdx.x] : blockIdx.x;      // the sub-queue this workgroup owns (input and output)
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    const ShadowLds sh = block_shadow_lds();
    STAGE_SMALL_TABLES(T, sc);
    const uint32_t G = gridDim.x;
    uint32_t n = qrows[(size_t)bounce_first * G + qid];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const size_t qb = (size_t)qid * f.qcap;
    const uint32_t stride = COMPACT ? state_set_stride(p) : 0u;
    uint32_t par = 0;
    PF_BEGIN;
    for (uint32_t bounce = bounce_first; bounce < bounce_end; bounce++) {      // (launched for bounce 0 alone)
        const bool last = (bounce + 1u == f.max_bounces);
        const uint32_t sbounce = HAVE_HIT == 2 ? 0u : bounce;     // what the shading sees: with the literal 0 its MIS and Russian-roulette branches fold away
        const uint32_t* myq = ((bounce & 1u) ? queue_b : queue_a) + qb;
        uint32_t* mynext = ((bounce & 1u) ? queue_a : queue_b) + qb;
        for (uint32_t base = 0; base < n; base += kBlock) {       // one trip per 256 queue entries
            PF_MARK(0);
            PathState S = unspecified_path(); Surf sf = unspecified_surf();            // the lane's item: path, surface, hit (prim marks a lane without one: the rest is read beside a real prim only)
            float t = unspecified<float>(), u = unspecified<float>(), v = unspecified<float>(); uint32_t prim = kMissPrim;
            const uint32_t i = base + threadIdx.x;
            const bool active = i < n;
            if constexpr (HAVE_HIT == 2) {
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
            } else {
                if (active) { S = load_path(p, myq[i]); const F4 h = p.hit[S.pid]; t = h.x; u = h.y; v = h.z; prim = f2u(h.w); }
            }
            PF_MARK(2);
            shade_block<HAVE_HIT, LAMBERT, COMPACT>(sc, small, L, f, p, T, sh, par, S, sf, t, u, v, prim, active, sbounce, nee, last, s_cnt, mynext, state_out((uint32_t)qb, stride, bounce), pf);
        }
        n = end_bounce<false>(s_cnt, nullptr, qrows, srows, bounce, G, qid, nee);
    }
    PF_FLUSH;
}

// ---- bounces >= 1, scheduled per workgroup (RTX_OPT_BOUNCE_VARIANT 0 / 1) ----
// These two bodies keep the path state by path id, in place: a frame that runs one of them uses that layout throughout, bounce 0 included (plan_batches, rtx_render.hip).
// RING: 1 = workgroup-wide LDS hit ring between trace and shading (variant 0); 0 = trace and shade the same 256 entries (variant 1)
template <bool LAMBERT, int RING>
__device__ __forceinline__ void bounce_small_block(const DevScene& sc, const SmallRecPair* small, const DevFrame& f_in, const DevPaths& p, uint32_t bounce_first, uint32_t bounce_end,
                                                   uint32_t* queue_a, uint32_t* queue_b, uint32_t* qrows, uint32_t* srows, const uint32_t* order) {
    extern __shared__ F4 lds[];
    __shared__ uint32_t s_cnt[1 + kMaxNee];
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);
    const uint32_t qid = order ? order[blockIdx.x] : blockIdx.x;
    wave_stamp(0u);
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    const ShadowLds sh = block_shadow_lds();
    STAGE_SMALL_TABLES(T, sc);
    const uint32_t G = gridDim.x;
    uint32_t n = qrows[(size_t)bounce_first * G + qid];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const size_t qb = (size_t)qid * f.qcap;
    uint32_t par = 0;
    PF_BEGIN;
    for (uint32_t bounce = bounce_first; bounce < bounce_end; bounce++) {
        const bool last = (bounce + 1u == f.max_bounces);
        const float tmin = bounce_tmin(bounce);
        const uint32_t* myq = ((bounce & 1u) ? queue_b : queue_a) + qb;
        uint32_t* mynext = ((bounce & 1u) ? queue_a : queue_b) + qb;
        if constexpr (!RING) {
            for (uint32_t base = 0; base < n; base += kBlock) {   // one trip per 256 queue entries: lanes whose ray missed idle through the shading
                PF_MARK(0);
                PathState S = unspecified_path(); Surf sf = unspecified_surf();            // the lane's item: path, surface, hit (prim marks a lane without one: the rest is read beside a real prim only)
                float t = unspecified<float>(), u = unspecified<float>(), v = unspecified<float>(); uint32_t prim = kMissPrim;
                const uint32_t i = base + threadIdx.x;
                const bool active = i < n;
                if (active) S = load_path(p, myq[i]);
                traverse_small<false, true>(sc, small, L, S.o, S.d, tmin, active ? kTMax : 0.0f, t, u, v, prim, sc.nsmall, ~0ull, pf, 1);   // inactive lanes: empty interval
                PF_MARK(2);
                shade_block<0, LAMBERT, false>(sc, small, L, f, p, T, sh, par, S, sf, t, u, v, prim, active, bounce, nee, last, s_cnt, mynext, 0u, pf);
            }
        } else {
            // HIT RING.  20-25 % of the extension rays of a bounce leave the open front of the box or end on the light, and their lanes used to idle
            // through surface reconstruction, NEE and BSDF sampling — over half of the kernel's instructions (46-47 of 64 lanes active per VALU instruction,
            // profiles/r02_pmc_cornell.md).  Tracing and shading are therefore decoupled inside the workgroup: the trace phase takes 256 queue entries at a time
            // and pushes only the HITS (path slot + hit record, 20 B) into an LDS ring (ballot + one LDS atomic per wave); whenever the ring holds a full 256 (or
            // the input is exhausted) the shading phase runs on ring entries, i.e. on full waves.  A miss costs nothing beyond its trace.  The price: the path state
            // is read twice (origin / direction for the trace, all 48 B for the shading), which a VALU-bound kernel at 2.4 of 8 TB/s does not notice.
            // All four waves walk through the same phases (every decision is read from LDS after a barrier), so there is no producer / consumer protocol.
            constexpr uint32_t kRing = 512u;                       // < 256 waiting + <= 256 pushed by one trace pass
            __shared__ uint32_t s_rpid[kRing];
            __shared__ F4 s_rhit[kRing];
            // Ring counters.  s_ring[0] = entries consumed (written by thread 0 between two barriers).  Entries PRODUCED are counted per trace pass in one of three
            // rotating LDS words (pass k pushes into s_rc[k % 3]) and summed in a register (`prod`) after the barrier that ends the pass: the loop condition below then
            // depends on registers and on s_ring[0] only, never on a word another wave may be pushing into.  (With ONE produced-counter read in the condition, a wave
            // that evaluated it late could see a push of the current pass, leave the loop and strand the others at the barrier — a formal race)  A word is
            // cleared by thread 0 after the barrier of pass k + 1 and next pushed into in pass k + 3; it was last read before that barrier.
            __shared__ uint32_t s_ring[1], s_rc[3];
            if (threadIdx.x < 3) s_rc[threadIdx.x] = 0;
            if (threadIdx.x == 3) s_ring[0] = 0;
            __syncthreads();
            uint32_t next_in = 0;                                   // trace phase: next input entry (uniform)
            uint32_t prod = 0, rk = 0;                              // hits pushed by the completed trace passes of this bounce; pass number mod 3 (both uniform)
            for (;;) {                                              // one trip per 256 ring entries, until input and ring are empty
                PF_MARK(0);
                PathState S = unspecified_path(); Surf sf = unspecified_surf();            // the lane's item: path, surface, hit (prim marks a lane without one: the rest is read beside a real prim only)
                float t = unspecified<float>(), u = unspecified<float>(), v = unspecified<float>(); uint32_t prim = kMissPrim;
                // ---- trace phase: fill the ring until it holds a full workgroup of hits (or the input runs out) ----
                while (next_in < n && prod - s_ring[0] < kBlock) {                // uniform: `prod` is a register, s_ring[0] was written before the last barrier
                    const uint32_t i = next_in + threadIdx.x;
                    const bool act = i < n;
                    uint32_t pid = unspecified<uint32_t>(); f3 ro = unspecified3(), rd = unspecified3();      // a lane without an entry: pid is read under `hit` only, its ray has tmax = 0
                    if (act) { pid = myq[i]; const F4 a = p.ray_o[pid], b = p.ray_d[pid]; ro = mk3(a.x, a.y, a.z); rd = mk3(b.x, b.y, b.z); }
                    float ht, hu, hv; uint32_t hp;
                    traverse_small<false, true>(sc, small, L, ro, rd, tmin, act ? kTMax : 0.0f, ht, hu, hv, hp, sc.nsmall, ~0ull, pf, 1);   // inactive lanes: empty interval
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
                const bool active = threadIdx.x < take;
                if (active) {
                    const uint32_t e = (head + threadIdx.x) & (kRing - 1u);
                    S = load_path(p, s_rpid[e]);
                    const F4 h = s_rhit[e]; t = h.x; u = h.y; v = h.z; prim = f2u(h.w);
                }
                __syncthreads();                                                    // every lane has read its entry before the slots are released
                if (threadIdx.x == 0) s_ring[0] = head + take;
                PF_MARK(2);
                shade_block<0, LAMBERT, false>(sc, small, L, f, p, T, sh, par, S, sf, t, u, v, prim, active, bounce, nee, last, s_cnt, mynext, 0u, pf);
                __syncthreads();                                    // the released ring slots (s_ring[0]) are visible to the next trip's trace phase
            }
        }
        n = end_bounce<false>(s_cnt, nullptr, qrows, srows, bounce, G, qid, nee);
    }
    PF_FLUSH;
    wave_stamp(1u);
}

// Fused bounce kernel for tiny scenes (sc.nsmall != 0): trace the extension ray, shade, trace the NEE shadow
// rays and add their contributions, sample the BSDF, compact — all in one pass over the workgroup's sub-queue.
// Nothing but the 48-B path state and the queue index moves through HBM; hit records and shadow-ray entries
// stay in registers.
// COMPACT: the path state lives by queue position in two sets instead of by path id (rtx_bounce_small_parts.hpp); bounce 0 and the wave-scheduled body (RING 2) have both forms.
// BOUNCE RANGE: sub-queues are workgroup-private, so bounce b + 1 of sub-queue q depends on bounce b of the SAME sub-queue only.  One
// launch therefore runs the bounces [bounce_first, bounce_end) of its sub-queue back to back, with a workgroup barrier in between
// (workgroup-scope release / acquire: the path state and queue entries a bounce writes are read by the same workgroup: end_bounce).  A frame has
// two fused launches (bounce 0, which reads the primary hits, and bounces 1 .. max_bounces - 1) instead of eight, and no drain /
// ramp-up between the bounces; the sparsely populated late bounces cost a few loop trips instead of a launch each.
// LAMBERT: RTX_FLAG_LAMBERT_ONLY is a launch constant, so it is a template parameter too: the Lambert-only instantiation carries no GGX code
// (fewer live registers, fewer SGPR spills through v_writelane / v_readlane in the loop).
// HAVE_HIT: 0 = bounces >= 1 (the kernel traces its extension rays); 1 / 2 = bounce 0, the two inputs of bounce_small_first
// RING (bounces >= 1, RTX_OPT_BOUNCE_VARIANT 0 / 1 / 2 = RING 1 / 0 / 2): 0 / 1 = the two forms of bounce_small_block; 2 = bounce_small_wave: wave-private buffers, no barrier inside a bounce
template <int WAVES, int HAVE_HIT, bool LAMBERT, int RING, bool COMPACT>
__global__ __launch_bounds__(kBlock, WAVES) void k_bounce_small(DevScene sc, const SmallRecPair* __restrict__ small, DevFrame f_in, DevPaths p,
                                                         uint32_t bounce_first, uint32_t bounce_end,
                                                         uint32_t* __restrict__ queue_a, uint32_t* __restrict__ queue_b /* bounce b reads (b & 1 ? b : a), writes the other */,
                                                         uint32_t* __restrict__ qrows /* [bounce][gridDim.x] sub-queue lengths entering each bounce */,
                                                         uint32_t* __restrict__ srows /* [bounce][nee][gridDim.x]: shadow rays traced (statistics) */,
                                                         const uint32_t* __restrict__ order /* workgroup -> sub-queue, longest first (k_order_queues); may be null */,
                                                         PrimIn pin /* HAVE_HIT 2: the per-pixel records of k_primary_surface and how to find a path's (read by that instantiation only) */) {
    static_assert(HAVE_HIT == 0 || RING == 0, "bounce 0 has no extension trace, hence no ring: launch_bounce_small");
    static_assert(!COMPACT || HAVE_HIT != 0 || RING == 2, "the block-scheduled bodies keep the path state in place: launch_bounce_small");
    if constexpr (HAVE_HIT != 0) bounce_small_first<HAVE_HIT, LAMBERT, COMPACT>(sc, small, f_in, p, bounce_first, bounce_end, queue_a, queue_b, qrows, srows, order, pin);
    else if constexpr (RING == 2) bounce_small_wave<LAMBERT, COMPACT>(sc, small, f_in, p, bounce_first, bounce_end, queue_a, queue_b, qrows, srows, order);
    else bounce_small_block<LAMBERT, RING>(sc, small, f_in, p, bounce_first, bounce_end, queue_a, queue_b, qrows, srows, order);
}

}  // namespace rtx

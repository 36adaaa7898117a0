// rtx_k_bounce_wave.hpp — the wave-private form of the fused tiny-scene bounce kernel (k_bounce_small<.., 0, .., RING = 2>, RTX_OPT_BOUNCE_VARIANT = 2)
// One of the kernel headers of rtx_kernels.hip; included by rtx_k_bounce_small.hpp, whose kernel calls bounce_small_wave() as its whole body for RING == 2.
// What it shares with the other two bodies (table staging, hit -> shading decision, continuation, bounce end, ...) is defined once, in rtx_bounce_small_parts.hpp.
// Uses the PF_* section-profile macros that rtx_kernels.hip defines before it includes the kernel headers.
#pragma once
#include "rtx_bounce_small_parts.hpp"

namespace rtx {

// LDS written by some lanes of a wave and read by others of the SAME wave: the hardware executes a wave's LDS instructions in order, so all that is needed is that the
// compiler keeps the program order of the accesses (wavefront-scope fences emit no instruction)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Bounces [bounce_first, bounce_end), bounce_first >= 1, of the workgroup's sub-queue — the same work, arithmetic and radiance order as bounce_small_block<.., 1> (rtx_k_bounce_small.hpp),
// scheduled per WAVE instead of per workgroup: inside a bounce no wave ever waits for another.
//   input     a wave takes the next 64 queue entries from an LDS cursor (s_in, one atomic per chunk): the four waves stay balanced whatever their rays cost
//   hit buffer  per wave, 64 entries (path id — COMPACT: the entry's place in the input queue — + hit record) in LDS that only this wave touches; a trace pass pushes its hits with ballot + mbcnt at a wave-uniform
//             count held in a register (no LDS atomic).  The wave traces until it has >= 64 hits or the input is exhausted, then shades min(64, avail) entries.  A pass that
//             takes the count to 64 + r keeps its last r hits in registers until the 64 buffered ones are popped (a few instructions later) and then writes them to slots 0 .. r - 1:
//             what a 128-entry ring would hold, in half the LDS — with 64-entry buffers the Lambert instantiation keeps five workgroups per CU, with 128-entry rings it would run three
//   shadow    nee_sample's rays go into a second wave-private buffer of 64 entries (origin + tmin flag, direction + tmax, contribution + path id), filled the same
//             way; when a push takes it to 64 the wave traces one FULL block and every lane whose ray is unoccluded adds its entry's contribution to that path's radiance (a plain
//             read-modify-write), then the rest of the push goes to the front of the emptied buffer.
//             A path has at most one pending entry per block: with nee_samples == 1 by construction (one push per path and bounce); with nee_samples > 1 the buffer is drained after
//             every NEE slot's push, before slot j + 1 pushes, so a path's slots are added in order and never by two lanes at once.  The buffer is drained, as a partial block,
//             before the wave leaves the bounce: with the bounce-end barrier, a path's additions of bounce b are complete before bounce b + 1 reads its radiance — the oracle's
//             order (emissive, NEE slot 0, 1, ..., next bounce).  An emissive hit and an NEE entry of the same path cannot coexist within a bounce (add_emissive XOR shading).
//             (An immediate form — no shadow buffer, the wave traces its shadow rays right after nee_sample at the 2/3 of the lanes that pushed — measured slower: docs/REJECTED.md.)
// INVARIANTS.  (1) Barriers: the only workgroup barriers are the table-staging one and the three at each bounce boundary (end_bounce: end of bounce, counters published, counters reset);
// every wave executes each exactly once per bounce, outside every data-dependent loop.  There is no producer / consumer protocol between waves.  (2) Termination: every loop ends
// because the input cursor only grows (a wave that reads a cursor >= n never asks again in this bounce) and a buffer only drains once the input is exhausted (each trip of the
// outer loop pops >= 1 entry of the hit buffer or ends the bounce; a shadow block empties the shadow buffer).
// COMPACT (rtx_bounce_small_parts.hpp): the path state lives by queue position in two sets.  The trace phase fetches origin and direction of entry i at in0 + i — no queue read
// before the ray fetch — and the hit buffer carries i; the shading phase loads the 48-B state at in0 + i and the path id, myq[i], which the radiance additions and the next
// queue's entry need; a survivor's state goes to out0 + its slot in the next queue.
template <bool LAMBERT, bool COMPACT>
__device__ __forceinline__ void bounce_small_wave(const DevScene& sc, const SmallRecPair* __restrict__ small, const DevFrame& f_in, const DevPaths& p, uint32_t bounce_first, uint32_t bounce_end,
                                                  uint32_t* __restrict__ queue_a, uint32_t* __restrict__ queue_b, uint32_t* __restrict__ qrows, uint32_t* __restrict__ srows, const uint32_t* __restrict__ order) {
    extern __shared__ F4 lds[];
    constexpr uint32_t kWaves = kBlock / 64u, kHitBuf = 64u, kShBuf = 64u;
    __shared__ uint32_t s_cnt[1 + kMaxNee];
    __shared__ uint32_t s_in;                                          // input cursor of the bounce: next unclaimed queue entry
    __shared__ uint32_t s_hpid[kWaves * kHitBuf];
    __shared__ F4 s_hhit[kWaves * kHitBuf];
    __shared__ F4 s_so[kWaves * kShBuf], s_sd[kWaves * kShBuf], s_sc[kWaves * kShBuf];
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);
    const uint32_t qid = order ? order[blockIdx.x] : blockIdx.x;
    wave_stamp(0u);
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_in = 0;
    STAGE_SMALL_TABLES(T, sc);
    const uint32_t G = gridDim.x;
    uint32_t n = qrows[(size_t)bounce_first * G + qid];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const size_t qb = (size_t)qid * f.qcap;
    const uint32_t stride = COMPACT ? state_set_stride(p) : 0u;
    const uint32_t lane = lane_id();
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t* const hpid = s_hpid + wv * kHitBuf; F4* const hhit = s_hhit + wv * kHitBuf;      // this wave's buffers
    F4* const sho = s_so + wv * kShBuf; F4* const shd = s_sd + wv * kShBuf; F4* const shc = s_sc + wv * kShBuf;
    PF_BEGIN;
    for (uint32_t bounce = bounce_first; bounce < bounce_end; bounce++) {
        const bool last = (bounce + 1u == f.max_bounces);
        const float tmin = bounce_tmin(bounce);
        const uint32_t* myq = ((bounce & 1u) ? queue_b : queue_a) + qb;
        uint32_t* mynext = ((bounce & 1u) ? queue_a : queue_b) + qb;
        const uint32_t in0 = state_in((uint32_t)qb, stride, bounce), out0 = state_out((uint32_t)qb, stride, bounce);      // COMPACT: this sub-queue's first entry in the set read / written
        uint32_t hcnt = 0;                                          // hit buffer: entries waiting (wave-uniform register; < 64 between trace passes)
        uint32_t shcnt = 0;                                         // lane j: shadow rays this wave pushed for NEE slot j in this bounce
        bool in_done = false;                                       // this wave has seen the cursor at or past n
        uint32_t scnt = 0;                                          // shadow buffer, likewise
        // trace the first k <= 64 entries of the shadow buffer (all it holds) and add the unoccluded contributions
        auto shadow_block = [&](uint32_t k) {
            wave_lds_sync();                                        // the pushes are visible to the lanes that trace them
            const bool mine = lane < k;
            const uint32_t e = lane;
            F4 ro = unspecified4(), rd = unspecified4();         // a lane beyond the block: any ray, with an empty interval (its candidates are cleared) and no say in the record count
            if (mine) { ro = sho[e]; rd = shd[e]; }
            float st_, su_, sv_; uint32_t sprim;
            traverse_small<true, false, true>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), fabsf(ro.w), mine ? rd.w : 0.0f, st_, su_, sv_, sprim, shadow_records(sc, mine, ro.w), ~0ull, pf, 6);
            if (mine && sprim == kMissPrim) {
                const F4 c = shc[e];
                const uint32_t pid = f2u(c.w);
                F4 radv = p.rad[pid];      // (issued before the traversal instead, for every lane of the block: 4 more live VGPRs, measured the same — docs/REJECTED.md)
                radv.x = radv.x + c.x; radv.y = radv.y + c.y; radv.z = radv.z + c.z;
                p.rad[pid] = radv;
            }
            wave_lds_sync();                                        // the entries are read before a later push reuses their slots
            PF_MARK(8);
        };
        for (;;) {
            PF_MARK(0);
            // ---- trace phase: trace input chunks until this wave has a full wave of hits (or the input runs out) ----
            bool full = false, carry = false;                        // full (uniform): the last pass took the count to 64 or more; carry: this lane's hit of that pass is beyond slot 63
            // the carried hit is read under `carry` only, and a pass that sets carry writes all six
            uint32_t cpid = unspecified<uint32_t>(), cprim = unspecified<uint32_t>(), ce = unspecified<uint32_t>(), hnext = 0; float ct = unspecified<float>(), cu = unspecified<float>(), cv = unspecified<float>();
            while (!in_done && !full) {
                uint32_t c0 = 0;
                if (lane == 0) c0 = atomicAdd(&s_in, 64u);
                c0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)c0);
                if (c0 >= n) { in_done = true; break; }
                const uint32_t i = c0 + lane;
                const bool act = i < n;
                uint32_t pid = unspecified<uint32_t>(); f3 ro = unspecified3(), rd = unspecified3();      // pid: what the hit buffer carries — the path id, or (COMPACT) the entry's place in the queue; a lane without an entry: read under `hit` only, its ray has tmax = 0
                if (act) { pid = COMPACT ? i : myq[i]; const uint32_t src = COMPACT ? in0 + i : pid; const F4 a = p.ray_o[src], b = p.ray_d[src]; ro = mk3(a.x, a.y, a.z); rd = mk3(b.x, b.y, b.z); }
                float ht, hu, hv; uint32_t hp;
                traverse_small<false, true>(sc, small, L, ro, rd, tmin, act ? kTMax : 0.0f, ht, hu, hv, hp, sc.nsmall, ~0ull, pf, 1);   // inactive lanes: empty interval
                const bool hit = act && hp != kMissPrim;
                const unsigned long long hmask = __ballot(hit);
                const uint32_t e = hcnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(hmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hmask, 0u));
                if (hit && e < kHitBuf) { hpid[e] = pid; hhit[e] = {ht, hu, hv, u2f(hp)}; }
                const uint32_t tot = hcnt + (uint32_t)__popcll(hmask);        // < 64 waiting + <= 64 pushed
                if (tot >= kHitBuf) { full = true; hnext = tot - kHitBuf; carry = hit && e >= kHitBuf; ce = e - kHitBuf; cpid = pid; ct = ht; cu = hu; cv = hv; cprim = hp; }
                else hcnt = tot;
            }
            const uint32_t take = full ? 64u : hcnt;
            if (take == 0u) break;                                  // input exhausted and buffer drained: this wave is done with the bounce
            const bool active = lane < take;
            PathState S = unspecified_path();
            float t = unspecified<float>(), u = unspecified<float>(), v = unspecified<float>(); uint32_t prim = kMissPrim;      // prim marks the lane idle; the rest is read beside a real prim only
            wave_lds_sync();                                        // the pushes above are visible to the lanes that pop them
            if (active) {
                const uint32_t e = hpid[lane];
                S = load_path(p, COMPACT ? in0 + e : e);
                if (COMPACT) S.pid = myq[e];
                const F4 h = hhit[lane]; t = h.x; u = h.y; v = h.z; prim = f2u(h.w);
            }
            wave_lds_sync();                                        // every lane has read its entry before the slots are written again
            if (carry) { hpid[ce] = cpid; hhit[ce] = {ct, cu, cv, u2f(cprim)}; }      // the hits of the last pass beyond the 64 just popped: the front of the emptied buffer
            hcnt = full ? hnext : 0u;
            PF_MARK(2);
            // ---- shading: the steps of shade_block (rtx_k_bounce_small.hpp), the shadow rays into this wave's buffer ----
            Surf sf = unspecified_surf();
            bool shading = false;
            if (active && prim != kMissPrim) { PF_COUNT(3); shading = hit_to_shading<0>(sc, p, T.mats, S, sf, t, u, v, prim, bounce, nee); }
            const f3 outgoing = -S.d, pos = sf.pos;
            const MatGPU* mp = T.mats + (shading ? sf.mat : 0u);
            f3 normal = sf.normal;
            const float eta_p = LAMBERT ? 0.0f : transmission_eta(*mp, f.flags, outgoing, normal);
            PF_MARK(3);
            for (uint32_t j = 0; j < nee; j++) {
                bool push = false;
                F4 so, sd; f3 con;                                 // no initialiser: every read is under `push`, and nee_sample assigns all three before it returns true
                if (shading) { PF_COUNT(4); push = nee_sample(sc, *mp, f.flags, nee, S, pos, normal, outgoing, so, sd, con, sf.near_hull, eta_p, nullptr, T.cdf, T.lights); }
                PF_MARK(4);
                const unsigned long long pmask = __ballot(push);
                const uint32_t npush = (uint32_t)__popcll(pmask);
                if (lane == j) shcnt += npush;
                const uint32_t e = scnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(pmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pmask, 0u));
                if (push && e < kShBuf) { sho[e] = so; shd[e] = sd; shc[e] = {con.x, con.y, con.z, u2f(S.pid)}; }
                const uint32_t tot = scnt + npush;                  // < 64 waiting + <= 64 pushed
                PF_MARK(5);
                if (tot >= kShBuf) {                               // a full block: trace it, then the rest of this push goes to the front of the emptied buffer
                    shadow_block(kShBuf);
                    if (push && e >= kShBuf) { sho[e - kShBuf] = so; shd[e - kShBuf] = sd; shc[e - kShBuf] = {con.x, con.y, con.z, u2f(S.pid)}; }
                    scnt = tot - kShBuf;
                } else scnt = tot;
                if (nee > 1u && scnt) { shadow_block(scnt); scnt = 0; }        // drain per slot: slot j + 1 of a path is pushed after slot j was added
            }
            continue_path<COMPACT>(*mp, f, p, bounce, shading && !last, S, pos, normal, outgoing, eta_p, &s_cnt[0], mynext, out0, pf);
            PF_MARK(9);
        }
        if (scnt) { shadow_block(scnt); scnt = 0; }                 // the partial block: nothing of this bounce stays pending
        if (lane < nee && shcnt) atomicAdd(&s_cnt[1u + lane], shcnt);
        n = end_bounce<true>(s_cnt, &s_in, qrows, srows, bounce, G, qid, nee);
    }
    PF_FLUSH;
    wave_stamp(1u);
}

}  // namespace rtx

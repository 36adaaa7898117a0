// rtx_k_shade.hpp — the shading kernels of the general path (the device functions they call: rtx_shade.hpp)
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
// Uses the PF_* section-profile macros that rtx_kernels.hip defines before it includes this file.
#pragma once
#include "rtx_shade.hpp"
#include "rtx_normalmap.hpp"
#include "rtx_specmap.hpp"

namespace rtx {

// shade: one thread per queued path (general path: hits come from k_trace_closest, shadow rays go to queues).
// SORT = material-sorted shading: the workgroup's sub-queue is consumed in chunks of kSortChunk entries; each chunk is
// counting-sorted in LDS by the material id of the hit (misses last), so that a wave shades ONE material and its
// branches (emissive / Lambert / GGX strategy, miss) are wave-uniform.  The sort never leaves LDS: the queue index and
// the hit record it reads are needed by the shading anyway.  Results do not depend on the order (per-path state only).
// MEASURED (MI355X, 1080p 16 spp 8 bounces, ms per 2 frames in k_shade): Bistro-class (30 % GGX) 18.1 unsorted vs 23.3
// sorted, Sponza-class 16.1 vs 32.1 — k_shade is HBM-bound, not divergence-bound, and the permutation turns its
// coalesced per-path state streams into gathers; k_trace_shadow gains 4-8 % from the more coherent shadow rays, the
// frame loses 1-10 %.  Round 2, with the path state kept by queue position (the permutation then stays inside a 2048-entry window of
// each stream): still slower, k_shade per frame 7.4 -> 10.6 ms (Sponza-class), 8.6 -> 9.8 ms (Bistro-class, where k_shade is VALU-bound at
// 33 of 64 lanes).  Hence RTX_OPT_SORT_MATERIALS defaults to 0.
// One item of k_shade / k_shade_dense: entry `qi` of the workgroup's sub-queue (valid = the lane has one).  Every lane of the wave goes through the compactions.
// (Phase 2 of k_bounce_bvh is a copy of this body without the compact state, the sort keys and MixView — calling it there measured slower: change the two together.)
// TEX: some material has a diffuse texture map (rtx_texture.hpp): Kd' / PI of the hit is formed once, after surface(), and handed to the mixture of the NEE samples and of the
// continuation — three floats live across them, no per-lane copy of the material.  Lanes whose material has no map keep its KdPi.
// ENV: an environment with weight is committed (rtx_env.hpp): a lane whose ray missed loads its path state and adds the map's radiance (env_miss), and every shading
// point casts one more NEE sample, towards the map, into shadow queue `nee` (env_marg: the marginal CDF, in LDS where k_shade found room).  ENV = false is the code as it was.
// NRM (implies TEX): some material has a normal map (rtx_normalmap.hpp): the shading normal of a lane that shades is perturbed once, right after surface(), and everything
// the lane does afterwards sees n' — three floats replaced, nothing more lives across the item.  NRM = false is the code as it was.
// SPC (implies TEX, never LAMBERT): some material has a specular, roughness or metalness map (rtx_specmap.hpp): Ks', Pr', Pm' of a lane that shades are formed once, next to
// Kd' and n', and handed to the view terms, the NEE samples and the continuation as kdpi is — five floats live across the item, and where a roughness map meets an energy
// table the view terms take their Ess from the table.  SPC = false is the code as it was.
// EMI (implies TEX): some emitter's material has an emission map (rtx_emimap.hpp): a lane that hits an emitter adds Ke' and weighs it by the triangle's q, and every
// triangle-light NEE sample multiplies the light's emission by the texel at the sampled point.  Nothing of it lives across the item.  EMI = false is the code as it was.
template <bool LAMBERT, bool TEX = false, bool ENV = false, bool NRM = false, bool SPC = false, bool EMI = false>
__device__ __forceinline__ void shade_item(const DevScene& sc, const DevFrame& f, const DevPaths& p, uint32_t bounce, uint32_t nee, bool last, size_t qb,
                                           const uint32_t* __restrict__ myq, uint32_t* __restrict__ mynext, uint32_t* s_cnt, bool valid, uint32_t qi, Prof* pf, const float* lds_cdf = nullptr, const LightGPU* lds_lights = nullptr, const MatGPU* lds_mats = nullptr, const float* env_marg = nullptr) {
    PathState S = idle_path();
    Surf sf = idle_surf();
    bool shading = false;
    f3 kdv = mk3(0, 0, 0); const f3* kdpi = TEX ? &kdv : nullptr;
    SpecView spv = {{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f}; const SpecView* sp = SPC ? &spv : nullptr;
    const float* ess_tab = nullptr;
#ifndef RTX_NO_LDS_MATS
    const MatGPU* mats = lds_mats ? lds_mats : sc.mats;      // (uniform; k_shade stages a short material table beside the light list)
#else
    const MatGPU* mats = sc.mats;
#endif
    if (valid) {
        const uint32_t pid = myq[qi];
        const uint32_t src = p.out_o ? (uint32_t)qb + qi : pid;               // compact state: hit and path state live at the queue position
        const F4 h = ld_stream(p.hit + src);
        const uint32_t prim = f2u(h.w);
        if (prim != kMissPrim) {                                          // miss: Miss.hlsl:3-11 -> black, terminate
            S = load_path_stream(p, src); S.pid = pid;
            PF_MARK(0); PF_COUNT(1);
            sf = surface(sc, S.o, S.d, h.x, h.y, h.z, prim);
            PF_MARK(1);
            if (sf.mat < sc.nmat) {
                const MatGPU& m = mats[sf.mat];
                if (m.Ke_len > 0.0f) {                                             // Hit.hlsl:126, Sampler_v6.hlsl:457
                    if (EMI) { const EmiHit eh = emi_hit(sc, m, sf.mat, prim, h.y, h.z); add_emissive(sc, p, S, sf, m, bounce, nee, false, &eh); }
                    else add_emissive(sc, p, S, sf, m, bounce, nee);
                }
                else { shading = true; if (TEX) kdv = tex_kdpi(sc, m, sf.mat, prim, h.y, h.z); if (NRM) sf.normal = nrm_perturb(sc, sf, prim, h.y, h.z, -S.d);
                       if (SPC) { spv = spec_view(sc, m, sf.mat, prim, h.y, h.z); ess_tab = spec_ess_table(sc, sf.mat); } }
            }
        }
        else if (ENV) { PathState M = load_path_stream(p, src); M.pid = pid; env_miss(sc, p, M, bounce); }      // the ray left the scene
    }
    const f3 outgoing = -S.d, pos = sf.pos;
    const MatGPU* mp = mats + (shading ? sf.mat : 0u);
    f3 normal = sf.normal;
    const float eta_p = LAMBERT ? 0.0f : transmission_eta(*mp, f.flags, outgoing, normal);          // (extension) hits from behind a dielectric flip the shading normal
    // the view-dependent terms of the mixture BSDF, once per shading point: the NEE samples and the continuation share them (rtx_bsdf.hpp: MixView)
    MixView mvs; const MixView* mv = nullptr;
#ifndef RTX_NO_MIXVIEW          // (A/B build: make VARIANT=nomv VARFLAGS=-DRTX_NO_MIXVIEW)
    if (!LAMBERT) { mvs = SPC ? mix_view(*mp, f.flags, normal, outgoing, eta_p, sp, ess_tab, sc.ess_rows) : mix_view(*mp, f.flags, normal, outgoing, eta_p); mv = &mvs; }
#endif
    PF_MARK(2);
    for (uint32_t j = 0; j < nee; j++) {                                  // NEE: visibility deferred to k_trace_shadow
        bool push = false;
        F4 so = {0, 0, 0, 0}, sd = {0, 0, 0, 0}; f3 con = mk3(0, 0, 0);
        if (shading) { PF_COUNT(3); }
        if (shading) push = nee_sample(sc, *mp, f.flags, nee, S, pos, normal, outgoing, so, sd, con, sc.nsmall != 0u && sf.near_hull, eta_p, mv, lds_cdf, lds_lights, kdpi, sp, EMI);
        PF_MARK(3);
        if (push) { PF_COUNT(4); }
        const size_t seg = (size_t)j * f.qcap * gridDim.x + qb;           // NEE slot j, this workgroup's sub-queue
        const uint32_t slot = block_push(push, &s_cnt[1 + j]);
        if (push) { st_stream(p.sh_o + seg + slot, so); st_stream(p.sh_d + seg + slot, sd); st_stream(p.sh_c + seg + slot, F4{con.x, con.y, con.z, u2f(S.pid)}); }
    }
    if (ENV) {                                                            // the environment's sample: NEE slot `nee`, after the triangle lights'
        bool push = false;
        F4 so = {0, 0, 0, 0}, sd = {0, 0, 0, 0}; f3 con = mk3(0, 0, 0);
        if (shading) push = env_nee_sample(sc, env_marg, *mp, f.flags, S, pos, normal, outgoing, so, sd, con, eta_p, mv, kdpi, sp);
        const size_t seg = (size_t)nee * f.qcap * gridDim.x + qb;
        const uint32_t slot = block_push(push, &s_cnt[1 + nee]);
        if (push) { st_stream(p.sh_o + seg + slot, so); st_stream(p.sh_d + seg + slot, sd); st_stream(p.sh_c + seg + slot, F4{con.x, con.y, con.z, u2f(S.pid)}); }
    }
    PF_MARK(4);
    bool alive = false;
    f3 smp = mk3(0, 0, 1); float P = 0.0f;
    if (shading && !last) { PF_COUNT(5); }
    if (shading && !last) alive = bsdf_continue(*mp, f, bounce, S, normal, outgoing, smp, P, eta_p, mv, kdpi, sp);
    PF_MARK(5);
    if (alive) { PF_COUNT(6); }
    const uint32_t slot = block_push(alive, &s_cnt[0]);
    if (alive) {
        if (p.out_o) store_path_at_stream(p.out_o, p.out_d, p.out_thr, (uint32_t)qb + slot, S, pos, smp, P);     // densely, at its place in the next queue
        else store_path(p, S, pos, smp, P);
        if (p.oct_out) {                                              // RTX_OPT_OCTANT_SORT: the key the next bounce's closest-hit kernel groups its fetches by
            uint32_t key = (f2u(smp.x) >> 31) | ((f2u(smp.y) >> 31) << 1) | ((f2u(smp.z) >> 31) << 2);            // 1: the direction octant (what ray_octant() will see: sign bits)
            if (p.key_mode == 3u) {                                   // 3: the cell of the ray's ORIGIN on a grid over the scene's box (sc.cell_*: 8 bits in all, split by the box's extents)
                const uint32_t bx = sc.cell_bits & 15u, by = (sc.cell_bits >> 4) & 15u, bz = (sc.cell_bits >> 8) & 15u;
                const uint32_t cx = (uint32_t)fminf(fmaxf((pos.x - sc.cell_o[0]) * sc.cell_s[0], 0.0f), (float)((1u << bx) - 1u));
                const uint32_t cy = (uint32_t)fminf(fmaxf((pos.y - sc.cell_o[1]) * sc.cell_s[1], 0.0f), (float)((1u << by) - 1u));
                const uint32_t cz = (uint32_t)fminf(fmaxf((pos.z - sc.cell_o[2]) * sc.cell_s[2], 0.0f), (float)((1u << bz) - 1u));
                key = cx | (cy << bx) | (cz << (bx + by));
            }
            if (p.key_mode == 5u) key = ((uint32_t)slot * 2654435761u) >> 24;      // 5 (tooling): a hashed key — the scattered fetch without any grouping, to price the fetch alone
            p.oct_out[qb + slot] = (uint8_t)key;
        }
        mynext[slot] = S.pid;
    }
}

constexpr uint32_t kSortChunk = 2048, kSortKeys = 64, kLdsCdf = 256;
// k_shade's dynamic LDS (launch and kernel agree through this one function): the light list (records + CDF) when it has <= 256 entries, the material table behind it while
// both stay within kShadeLds bytes.  RTX_SHADE_LDS (A/B builds) moves the budget; 0 = lights only.
#ifndef RTX_SHADE_LDS
#define RTX_SHADE_LDS 24576
#endif
constexpr uint32_t kShadeLds = RTX_SHADE_LDS;
__host__ __device__ inline void shade_lds_plan(uint32_t nlights, uint32_t nmat, bool sort, uint32_t& lights_bytes, uint32_t& mats_bytes) {
    lights_bytes = (!sort && nlights <= kLdsCdf) ? ((nlights * 84u + 15u) & ~15u) : 0u;
    mats_bytes = (!sort && nmat && lights_bytes + nmat * 160u <= kShadeLds) ? nmat * 160u : 0u;
}
#ifndef RTX_SHADE_WAVES
#define RTX_SHADE_WAVES 7          // waves per SIMD k_shade is compiled for: 7 = 72 VGPRs + 1 spilled (GGX) / 66 (Lambert); uncapped: 94 VGPRs, 5 waves; 6: 80, no spills; 8: 64, 9 spilled.
                                   // k_shade per frame, C3 / C5: 7.42 / 8.77 ms uncapped, 6.93 / 8.54 at 6, 7.50 / 8.83 at 8 (round 2); round 4: 6.27 / 6.85 at 6, 6.28 / 6.72 at 7
#endif
// the marginal CDF of the environment (<= 8 KB) behind the light list and the material table in k_shade<.., ENV>'s dynamic LDS, where the three stay within kShadeLds; else it is
// read from global memory like the conditional rows.  (A/B build: -DRTX_ENV_MARG_GLOBAL keeps it in global memory always.)
__host__ __device__ inline uint32_t shade_env_lds(uint32_t lights_bytes, uint32_t mats_bytes, uint32_t env_n) {
#ifdef RTX_ENV_MARG_GLOBAL
    return 0u;
#else
    return (env_n && lights_bytes + mats_bytes + env_n * 4u <= kShadeLds) ? ((env_n * 4u + 15u) & ~15u) : 0u;
#endif
}
#ifndef RTX_SHADE_WAVES_ENV
#define RTX_SHADE_WAVES_ENV 6      // ... of the ENV instantiations: the environment's sample lives beside the view terms of the mixture, and at 7 waves (72 VGPRs) the GGX forms spill 4 / 8 registers to scratch
#endif
#ifndef RTX_SHADE_WAVES_NRM
#define RTX_SHADE_WAVES_NRM 6      // ... of the NRM instantiations, with or without ENV (profiles/normalmap_kernel_resources.md)
#endif
#ifndef RTX_SHADE_WAVES_SPC
#define RTX_SHADE_WAVES_SPC 5      // ... of the SPC instantiations, with or without ENV / NRM (profiles/specmap_kernel_resources.md)
#endif
// ... of the EMI instantiations, with or without ENV / NRM (profiles/emimap_kernel_resources.md): the highest cap at which no form of the group spills a VGPR.  The light
// sample's texel fetch is live beside the mixture's terms: the GGX forms spill 3 - 7 registers at 6 waves, the SPC forms 1 at 5; the Lambert forms fit 6
#ifndef RTX_SHADE_WAVES_EMI
#define RTX_SHADE_WAVES_EMI 5
#endif
#ifndef RTX_SHADE_WAVES_EMI_LAMBERT
#define RTX_SHADE_WAVES_EMI_LAMBERT 6
#endif
#ifndef RTX_SHADE_WAVES_EMI_SPC
#define RTX_SHADE_WAVES_EMI_SPC 4
#endif
template <bool SORT, bool LAMBERT, bool TEX = false, bool ENV = false, bool NRM = false, bool SPC = false, bool EMI = false>     // LAMBERT: RTX_FLAG_LAMBERT_ONLY as a compile-time constant (no GGX / transmission code in that instantiation); TEX: texture maps, ENV: environment lighting, NRM: normal maps, SPC: specular maps, EMI: emission maps (shade_item)
__global__ __launch_bounds__(kBlock, (EMI ? (SPC ? RTX_SHADE_WAVES_EMI_SPC : LAMBERT ? RTX_SHADE_WAVES_EMI_LAMBERT : RTX_SHADE_WAVES_EMI) : SPC ? RTX_SHADE_WAVES_SPC : NRM ? RTX_SHADE_WAVES_NRM : ENV ? RTX_SHADE_WAVES_ENV : RTX_SHADE_WAVES)) void k_shade(DevScene sc, DevFrame f_in, DevPaths p, uint32_t bounce,
                                                  const uint32_t* __restrict__ queue, const uint32_t* __restrict__ qcount,
                                                  uint32_t* __restrict__ next_queue, uint32_t* __restrict__ next_count,
                                                  uint32_t* __restrict__ shcounts /* [nee][gridDim.x] */) {
    static_assert(!NRM || (TEX && !SORT), "the normal-mapped forms are TEX forms of the default kernel");
    static_assert(!SPC || (TEX && !SORT && !LAMBERT), "the specular-mapped forms are GGX TEX forms of the default kernel");
    static_assert(!EMI || (TEX && !SORT), "the emission-mapped forms are TEX forms of the default kernel");
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);
    constexpr uint32_t kSlots = kMaxNee + (ENV ? 1u : 0u);  // (the environment's slot follows the nee_samples <= kMaxNee triangle-light slots)
    __shared__ uint32_t s_cnt[1 + kMaxNee + (ENV ? 4u : 0u)];     // [0] next-queue length, [1 + j] shadow queue j length (ENV: one slot more, in a 16-byte step: the static LDS precedes the dynamic region, whose float4 reads need their alignment)
    __shared__ uint32_t s_pid[SORT ? kSortChunk : 1], s_sorted[SORT ? kSortChunk : 1], s_hist[SORT ? kSortKeys : 1];
    __shared__ uint8_t s_key[SORT ? kSortChunk : 1];
    // (round 5) a light list of <= 256 entries in LDS — the records (80 B each) and behind them the CDF: NEE's binary search is 1-8 DEPENDENT reads per sample (street scene:
    // 204 lights), the record one more.  Dynamic LDS, sized by the list at launch (shade_lds_bytes): a scene with two lights pays 168 bytes, not a workgroup per CU
    extern __shared__ F4 s_lights[];
    float* s_cdf = (float*)(s_lights + (size_t)sc.nlights * 5u);
    uint32_t lights_bytes, mats_bytes; shade_lds_plan(sc.nlights, sc.nmat, SORT, lights_bytes, mats_bytes);
    const bool cdf_in_lds = lights_bytes != 0u;
    if (cdf_in_lds) {
        for (uint32_t i = threadIdx.x; i < sc.nlights * 5u; i += kBlock) s_lights[i] = ((const F4*)sc.lights)[i];
        for (uint32_t i = threadIdx.x; i < sc.nlights; i += kBlock) s_cdf[i] = sc.cdf[i];
    }
    if (threadIdx.x <= kSlots) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const float* lds_cdf = cdf_in_lds ? s_cdf : nullptr;
    const LightGPU* lds_lights = cdf_in_lds ? (const LightGPU*)s_lights : nullptr;
    // ... and the material table (160 B each) behind the CDF when launch_shade found room for it (mats_in_lds: what it sized the dynamic LDS for)
    const MatGPU* lds_mats = nullptr;
    if (mats_bytes) {
        F4* dst = (F4*)((char*)s_lights + lights_bytes);
        for (uint32_t i = threadIdx.x; i < sc.nmat * 10u; i += kBlock) dst[i] = ((const F4*)sc.mats)[i];
        lds_mats = (const MatGPU*)dst;
    }
    const float* env_marg = nullptr;
    if (ENV) {
        env_marg = sc.env_marg;
        if (shade_env_lds(lights_bytes, mats_bytes, sc.env_n)) {
            float* dst = (float*)((char*)s_lights + lights_bytes + mats_bytes);
            for (uint32_t i = threadIdx.x; i < sc.env_n; i += kBlock) dst[i] = sc.env_marg[i];
            env_marg = dst;
        }
        __syncthreads();                                    // the copy (and the material table's above) is read by every wave
    }
    const uint32_t n = qcount[blockIdx.x];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const bool last = (bounce + 1u == f.max_bounces);
    const size_t qb = (size_t)blockIdx.x * f.qcap;
    const uint32_t* myq = queue + qb;
    uint32_t* mynext = next_queue + qb;
    const uint32_t chunk = SORT ? kSortChunk : n;
    PF_BEGIN;                                               // (PROFILE build: sections 0 load, 1 surface, 2 emissive / setup, 3 NEE sample, 4 shadow push, 5 BSDF sample, 6 store)
    for (uint32_t cb = 0; cb < n; cb += chunk) {
        const uint32_t cn = (n - cb < chunk) ? n - cb : chunk;
        if (SORT) {
            if (threadIdx.x < kSortKeys) s_hist[threadIdx.x] = 0;
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < cn; i += kBlock) {
                const uint32_t prim = f2u(p.hit[p.out_o ? (uint32_t)qb + cb + i : myq[cb + i]].w);
                const uint32_t key = prim == kMissPrim ? kSortKeys - 1u : (sc.shade[prim].mat % (kSortKeys - 1u));
                s_pid[i] = i; s_key[i] = (uint8_t)key;                 // (the entry's place in the chunk: the queue position is needed too)
                atomicAdd(&s_hist[key], 1u);
            }
            __syncthreads();
            if (threadIdx.x < 64) {                             // exclusive scan of the 64 bucket counts by one wave
                const uint32_t c = s_hist[threadIdx.x];
                uint32_t incl = c;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const uint32_t t = __shfl_up(incl, d); if ((int)threadIdx.x >= d) incl += t; }
                s_hist[threadIdx.x] = incl - c;
            }
            __syncthreads();
            for (uint32_t i = threadIdx.x; i < cn; i += kBlock) s_sorted[atomicAdd(&s_hist[s_key[i]], 1u)] = s_pid[i];
            __syncthreads();
        }
        for (uint32_t base = threadIdx.x & ~63u; base < cn; base += kBlock) {
            const uint32_t i = base + (threadIdx.x & 63u);
            shade_item<LAMBERT, TEX, ENV, NRM, SPC, EMI>(sc, f, p, bounce, nee, last, qb, myq, mynext, s_cnt, i < cn, cb + (SORT ? s_sorted[i] : i), pf, lds_cdf, lds_lights, lds_mats, env_marg);
        }
        if (SORT) __syncthreads();                              // the next chunk overwrites the LDS buffers
    }
    PF_MARK(6);
    PF_FLUSH;
    __syncthreads();
    if (threadIdx.x == 0) next_count[blockIdx.x] = s_cnt[0];
    if (threadIdx.x >= 1 && threadIdx.x <= nee + (ENV ? 1u : 0u)) shcounts[(size_t)(threadIdx.x - 1) * gridDim.x + blockIdx.x] = s_cnt[threadIdx.x];
}

// k_shade with the HITS of the sub-queue compacted before they are shaded (RTX_OPT_SHADE_DENSE).  In an open scene a large part of a bounce's rays leaves the scene
// (the Bistro-class street keeps 86 / 66 / 53 / 44 % of its paths through bounces 1-4) and in k_shade their lanes idle through surface reconstruction, NEE and BSDF
// sampling, which on that scene is VALU-bound work at 33 of 64 lanes (profiles/r02_pmc_bvh.md).  Here the workgroup reads the hit records of 256 entries at a time, pushes
// the entries that hit something into an LDS ring (ballot + one LDS atomic per wave), and shades ring entries 256 at a time — full waves of hits, as the hit ring of the
// fused tiny-scene kernel does.  The permutation stays inside the workgroup's sub-queue, so the state streams stay coalesced (monotone gathers within a 2-KB window; this is
// not the global material sort that was rightly rejected).  Same arithmetic per item; only the order of the entries in the next queue changes, which no result depends on.
// Ring bookkeeping as in k_bounce_small: hits of pass k are counted in s_blk[k % 3] and summed in a register after the pass's barrier, a word is cleared one pass later.
template <bool LAMBERT>
__global__ __launch_bounds__(kBlock, RTX_SHADE_WAVES) void k_shade_dense(DevScene sc, DevFrame f_in, DevPaths p, uint32_t bounce,
                                                        const uint32_t* __restrict__ queue, const uint32_t* __restrict__ qcount,
                                                        uint32_t* __restrict__ next_queue, uint32_t* __restrict__ next_count, uint32_t* __restrict__ shcounts) {
    const DevFrame f = frame_with_lambert<LAMBERT>(f_in);
    constexpr uint32_t kRing = 512u;
    __shared__ uint32_t s_cnt[1 + kMaxNee], s_list[kRing], s_blk[3];
    if (threadIdx.x <= kMaxNee) s_cnt[threadIdx.x] = 0;
    if (threadIdx.x < 3) s_blk[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t n = qcount[blockIdx.x];
    const uint32_t nee = sc.nlights ? f.nee_samples : 0u;
    const bool last = (bounce + 1u == f.max_bounces);
    const size_t qb = (size_t)blockIdx.x * f.qcap;
    const uint32_t* myq = queue + qb;
    uint32_t* mynext = next_queue + qb;
    Prof* pf = nullptr;
    uint32_t prod = 0, head = 0, rk = 0;                    // hits pushed / shaded so far, pass number mod 3 (all uniform, in registers)
    for (uint32_t base = 0; base < n; base += kBlock) {
        const uint32_t i = base + threadIdx.x;
        bool is_hit = false;
        if (i < n) is_hit = f2u(p.hit[p.out_o ? (uint32_t)qb + i : myq[i]].w) != kMissPrim;        // miss: Miss.hlsl:3-11 -> black, the path ends: nothing to do
        const uint32_t slot = prod + block_push(is_hit, &s_blk[rk]);
        if (is_hit) s_list[slot & (kRing - 1u)] = i;
        __syncthreads();
        prod += s_blk[rk];
        if (threadIdx.x == 0) s_blk[rk == 0u ? 2u : rk - 1u] = 0;
        rk = rk == 2u ? 0u : rk + 1u;
        const bool flush = base + kBlock >= n;
        while (prod - head >= (uint32_t)kBlock || (flush && prod != head)) {                      // uniform
            const uint32_t take = prod - head < (uint32_t)kBlock ? prod - head : (uint32_t)kBlock;
            const bool valid = threadIdx.x < take;
            const uint32_t qi = valid ? s_list[(head + threadIdx.x) & (kRing - 1u)] : 0u;
            shade_item<LAMBERT>(sc, f, p, bounce, nee, last, qb, myq, mynext, s_cnt, valid, qi, pf);
            head += take;
            __syncthreads();                                // every lane has read its ring slot before the next pass overwrites it
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) next_count[blockIdx.x] = s_cnt[0];
    if (threadIdx.x >= 1 && threadIdx.x <= nee) shcounts[(size_t)(threadIdx.x - 1) * gridDim.x + blockIdx.x] = s_cnt[threadIdx.x];
}

}  // namespace rtx

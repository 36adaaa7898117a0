// rtx_k_raygen.hpp — ray generation: the chunk deal into sub-queues, packet masks, the tiny scene's traced and shared primary hits
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
#pragma once
#include "rtx_shade.hpp"

namespace rtx {

// ---------------------------------------------------------------------------------------------
// raygen: one thread per path slot of the batch
// ---------------------------------------------------------------------------------------------
// LIST (all three raygen kernels): the frame's slot space is the active list of rtx_render_adaptive (real_slot, rtx_dev_common.hpp)
// LENS (the two that shoot camera rays): the thin-lens camera (camera_sample, rtx_dev_common.hpp); false = the pinhole, the kernels as they always were
template <bool LIST, bool LENS>
__global__ __launch_bounds__(kBlock) void k_raygen(DevFrame f, DevPaths p, const CameraGPU* __restrict__ cam_p, uint32_t* __restrict__ queue, uint32_t* __restrict__ qcount, uint32_t compact) {
    __shared__ CameraGPU cam;
    __shared__ uint32_t s_n;
    stage_camera(cam, cam_p);
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    uint32_t* myq = queue + (size_t)blockIdx.x * f.qcap;
    const uint32_t nchunks = f.chunks_per_sample * f.batch_spp;
    for (uint32_t k = 0, row0 = 0, c; row0 < nchunks; k++) {
        if (!dealt_chunk(f, k, row0, nchunks, c)) continue;
        uint32_t sl = c / f.chunks_per_sample, cl = c - sl * f.chunks_per_sample;         // wave-uniform (SALU)
        uint32_t pl = cl * kBlock + threadIdx.x;
        if (f.interleave) {                                                               // RTX_OPT_SAMPLE_INTERLEAVE: chunk = 256 / S pixel slots x S consecutive samples, the samples of a pixel in neighbouring
            const uint32_t sh = f.interleave, S = 1u << sh;                                  // lanes (S = 2 .. 16 divides batch_spp).  Changes no path (seeds come from pixel and sample id) and no sum (rad[] is per path)
            const uint32_t per = S * f.chunks_per_sample, sg = c / per, r = c - sg * per;
            sl = sg * S + (threadIdx.x & (S - 1u));
            pl = r * (kBlock >> sh) + (threadIdx.x >> sh);
        }
        const uint32_t pid = sl * f.npl + pl;
        uint32_t x = 0, y = 0;
        const bool valid = slot_to_pixel(f, real_slot<LIST>(f, pl), x, y);
        const uint32_t slot = block_push(valid, &s_n);
        if (valid) {
            uint32_t s0, s1; f3 o, d;
            camera_sample<LENS>(cam, f, x, y, f.sample_first + sl, o, d, s0, s1);
            const uint32_t dst = compact ? blockIdx.x * f.qcap + slot : pid;      // compact state: indexed by the queue position
            p.ray_o[dst] = {o.x, o.y, o.z, u2f(s1)};
            p.ray_d[dst] = {d.x, d.y, d.z, 1.0f};
            p.thr[dst] = {1.0f, 1.0f, 1.0f, u2f(s0)};
            p.rad[pid] = {0.0f, 0.0f, 0.0f, 0.0f};
            myq[slot] = pid;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) qcount[blockIdx.x] = s_n;
}

// packet-culling masks of the primary rays, one per 8x8 pixel block of the shard (slot order): they depend on the camera and the scene, not on the
// sample, so they are computed once per render call (one wave per block, lane = record) instead of once per block AND sample inside the raygen
// kernel, where they were more than half of its instructions (at 17 of 64 lanes)
__global__ __launch_bounds__(kBlock) void k_packet_masks(DevScene sc, DevFrame f, const CameraGPU* __restrict__ cam_p, unsigned long long* __restrict__ masks) {
    __shared__ CameraGPU cam;
    stage_camera(cam, cam_p);
    __syncthreads();
    const uint32_t blk = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);      // wave-uniform
    if (blk >= f.npl / 64u) return;
    uint32_t x = 0, y = 0;
    (void)slot_to_pixel(f, blk * 64u, x, y);                                    // slot 0 of the block = its top-left pixel
    const unsigned long long keep = packet_keep_mask(sc, cam, f, x & ~7u, y & ~7u);
    if (lane_id() == 0) masks[blk] = keep;
}

template <bool LIST, bool LENS>
__global__ __launch_bounds__(kBlock) void k_raygen_trace_small(DevScene sc, const SmallRecPair* __restrict__ small, DevFrame f, DevPaths p, const CameraGPU* __restrict__ cam_p,
                                                               uint32_t* __restrict__ queue, uint32_t* __restrict__ qcount, uint32_t* __restrict__ gencount,
                                                               const unsigned long long* __restrict__ masks /* k_packet_masks */) {
    extern __shared__ F4 lds[];
    __shared__ CameraGPU cam;
    __shared__ uint32_t s_n[2];
    stage_camera(cam, cam_p);
    if (threadIdx.x < 2) s_n[threadIdx.x] = 0;
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    uint32_t* myq = queue + (size_t)blockIdx.x * f.qcap;
    uint32_t generated = 0;
    const uint32_t nchunks = f.chunks_per_sample * f.batch_spp;
    // The deal, written out: it MUST equal dealt_chunk (rtx_dev_common.hpp) entry for entry — k_raygen_shared, which uses that, is correct only then.  (Through the helper the
    // compiler allocates this kernel's registers differently; the project keeps its device assembly fixed across refactors.)
    for (uint32_t k = 0, row0 = 0; row0 < nchunks; k++) {
        const uint32_t nk = f.taper_levels ? taper_row_width(k, gridDim.x, f.taper_levels) : gridDim.x;
        uint32_t pos = blockIdx.x;
        if (f.taper_levels && blockIdx.x < nk) { pos += (k * 2654435761u) % nk; if (pos >= nk) pos -= nk; }
        const uint32_t c = row0 + pos;
        row0 += nk;
        if (blockIdx.x >= nk || c >= nchunks) continue;                                   // wave-uniform
        const uint32_t sl = c / f.chunks_per_sample, cl = c - sl * f.chunks_per_sample;
        const uint32_t pl = real_slot<LIST>(f, cl * kBlock + threadIdx.x);       // the real slot: pixel, packet mask
        const uint32_t pid = sl * f.npl + cl * kBlock + threadIdx.x;
        uint32_t x = 0, y = 0, s0 = 0, s1 = 0;
        const bool valid = slot_to_pixel(f, pl, x, y);
        f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
        if (valid) {
            camera_sample<LENS>(cam, f, x, y, f.sample_first + sl, o, d, s0, s1);
            generated++;
        }
        // records that some ray of this wave's 8x8 pixel block can touch (slot_to_pixel lays one block out per wave): precomputed per block (LENS: all of them — the block's
        // pyramid from the camera origin does not bound rays that start elsewhere on the aperture, so the host fills the masks with ones instead of launching k_packet_masks)
        const unsigned long long km = masks[pl >> 6];
        const unsigned long long keep = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(km >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)km);
        float t, u, v; uint32_t prim;
        traverse_small<false, true>(sc, small, L, o, d, kTMinCam, valid ? kTMax : 0.0f, t, u, v, prim, sc.nsmall, keep);
        const bool hit = valid && prim != kMissPrim;
        // 43 % of the Cornell camera rays leave the box: their radiance stays zero, so only a hit bit is recorded for them
        const unsigned long long hm = __ballot(hit);
        if (lane_id() == 0) p.hitmask[pid >> 6] = hm;
        if (hit) {
            if (f.max_bounces == 0u) p.rad[pid] = {0.0f, 0.0f, 0.0f, 0.0f};   // otherwise the bounce-0 kernel writes every hit path's radiance slot
            p.ray_o[pid] = {o.x, o.y, o.z, u2f(s1)};
            p.ray_d[pid] = {d.x, d.y, d.z, 1.0f};
            p.thr[pid] = {1.0f, 1.0f, 1.0f, u2f(s0)};
            p.hit[pid] = {t, u, v, u2f(prim)};
        }
        const uint32_t slot = block_push(hit, &s_n[0]);
        if (hit) myq[slot] = pid;
    }
    atomicAdd(&s_n[1], generated);
    __syncthreads();
    if (threadIdx.x == 0) { qcount[blockIdx.x] = s_n[0]; gencount[blockIdx.x] = s_n[1]; }
}

// RTX_OPT_SHARED_PRIMARY.  Without RTX_FLAG_JITTER every sample of a pixel shoots the same camera ray, so its hit and the surface reconstructed there depend on the camera,
// the scene and the pixel only: they are computed ONCE per render call (one wave per 8x8 block, lane = pixel slot, the calls and arguments of k_raygen_trace_small and of the
// bounce-0 kernel, hence the same bits) and shared by all samples and batches of the call.  Record of slot pl, three streams of f.npl entries:
//   rec[pl] = (direction.xyz, material id | near_hull << 31)   rec[npl + pl] = (position.xyz, seed hash 1)   rec[2 npl + pl] = (normal.xyz, seed hash 0)   rec[3 npl] = (camera origin, -)
// (seed hashes: the pixel's terms of seed_init, seed_pixel; a material id is kept up to 2^31 - 1, beyond that it is no material's either way.)
// hits[blk] = the lanes of block blk whose ray hit something, hits[npl / 64 + blk] = the lanes that own a pixel; masks[blk] = the packet-culling mask (k_packet_masks: this
// kernel takes its place).
__global__ __launch_bounds__(kBlock) void k_primary_surface(DevScene sc, const SmallRecPair* __restrict__ small, DevFrame f, const CameraGPU* __restrict__ cam_p,
                                                            unsigned long long* __restrict__ masks, unsigned long long* __restrict__ hits, F4* __restrict__ rec) {
    extern __shared__ F4 lds[];
    __shared__ CameraGPU cam;
    stage_camera(cam, cam_p);
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const uint32_t pl = blockIdx.x * kBlock + threadIdx.x;                       // f.npl is a multiple of 256: every lane owns a slot
    if (pl >= f.npl) return;
    uint32_t x0 = 0, y0 = 0, x = 0, y = 0;
    (void)slot_to_pixel(f, pl & ~63u, x0, y0);                                   // slot 0 of the block = its top-left pixel
    const unsigned long long keep = packet_keep_mask(sc, cam, f, x0 & ~7u, y0 & ~7u);
    const bool valid = slot_to_pixel(f, pl, x, y);
    f3 o = mk3(0, 0, 0), d = mk3(0, 0, 1);
    if (valid) primary_ray(cam, f.width, f.height, x, y, 0.0f, 0.0f, o, d);
    float t, u, v; uint32_t prim;
    traverse_small<false, true>(sc, small, L, o, d, kTMinCam, valid ? kTMax : 0.0f, t, u, v, prim, sc.nsmall, keep);
    const bool hit = valid && prim != kMissPrim;
    const unsigned long long hm = __ballot(hit);
    const unsigned long long vm = __ballot(valid);
    if (lane_id() == 0) { masks[pl >> 6] = keep; hits[pl >> 6] = hm; hits[(f.npl >> 6) + (pl >> 6)] = vm; }
    if (pl == 0) rec[(size_t)3 * f.npl] = {cam.viewI[12], cam.viewI[13], cam.viewI[14], 0.0f};
    if (hit) {
        const Surf sf = surface(sc, o, d, t, u, v, prim);
        uint32_t h0, h1; seed_pixel(x, y, h0, h1);
        rec[pl] = {d.x, d.y, d.z, u2f((sf.mat < 0x7FFFFFFFu ? sf.mat : 0x7FFFFFFFu) | (sf.near_hull ? 0x80000000u : 0u))};
        rec[(size_t)f.npl + pl] = {sf.pos.x, sf.pos.y, sf.pos.z, u2f(h1)};
        rec[(size_t)2 * f.npl + pl] = {sf.normal.x, sf.normal.y, sf.normal.z, u2f(h0)};
    }
}

// the raygen of the shared-primary path: the chunk deal of k_raygen_trace_small (every sub-queue holds the same chunks in the same order), no trace, no path state and no pixel:
// whether a slot owns a pixel and whether its ray hit are two bits of the pre-pass (hits, k_primary_surface; nblk = the REAL frame's npl / 64), the same for every sample.
// A hitting path gets its queue entry — the path id — and nothing else: the bounce-0 kernel derives sample, slot and seeds from the id and the pixel's shared record, and
// k_accumulate takes the hit bit from hits[] too.  (rtx_render and rtx_render_adaptive refuse max_bounces == 0: bounce 0 always runs and writes every hit path's radiance slot.)
// NO SERIAL WALK.  A workgroup's ~50 chunks used to be one loop trip each — mask load, LDS atomic, store, every trip waiting for the one before: 0.34 ms of latency per frame for
// 0.3 GB of queue words.  Now the rows of the deal are taken 64 at a time: thread t owns block (t & 3) of row (t >> 2), finds its chunk in closed form (deal_row0, rtx_dev_common.hpp: the taper's
// widths repeat with period 2^(levels - 1)), loads its two mask words — all loads of the tile in flight together — and a workgroup scan of the popcounts places every block's
// entries; then each wave writes the entries of every fourth block from LDS.  Entries keep the chunk order of the serial walk, and inside a chunk the block order (the serial walk
// had the arrival order of its four waves there).
template <bool LIST>
__global__ __launch_bounds__(kBlock) void k_raygen_shared(DevFrame f, uint32_t* __restrict__ queue, uint32_t* __restrict__ qcount, uint32_t* __restrict__ gencount,
                                                          const unsigned long long* __restrict__ hits, uint32_t nblk) {
    __shared__ unsigned long long s_hm[kBlock];
    __shared__ uint32_t s_pid[kBlock], s_off[kBlock], s_wave[4], s_gen;
    if (threadIdx.x == 0) s_gen = 0;
    __syncthreads();
    uint32_t* myq = queue + (size_t)blockIdx.x * f.qcap;
    const uint32_t nchunks = f.chunks_per_sample * f.batch_spp;
    const uint32_t period = f.taper_levels ? 1u << (f.taper_levels - 1u) : 1u;
    uint32_t period_sum = 0;
    for (uint32_t j = 0; j < period; j++) period_sum += deal_width(f, j);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t generated = 0, qn = 0;                                                       // qn: entries written so far (uniform)
    for (uint32_t k0 = 0; deal_row0(f, k0, period, period_sum) < nchunks; k0 += 64u) {
        // ---- thread t: block (t & 3) of row k0 + (t >> 2): dealt_chunk with row0 in closed form ----
        const uint32_t k = k0 + (threadIdx.x >> 2);
        uint32_t row0 = deal_row0(f, k, period, period_sum), c;
        const bool dealt = dealt_chunk(f, k, row0, nchunks, c);
        unsigned long long hm = 0ull;
        uint32_t pid0 = 0;
        if (dealt) {
            const uint32_t sl = c / f.chunks_per_sample, cl = c - sl * f.chunks_per_sample;
            const uint32_t v = cl * kBlock + (threadIdx.x & 3u) * 64u;                  // first (virtual) slot of the block
            const uint32_t blk = real_slot<LIST>(f, v) >> 6;                            // the masks' index: real slots
            hm = hits[blk];                                                               // (a set bit implies a valid slot)
            generated += (uint32_t)__popcll(hits[nblk + blk]);
            pid0 = sl * f.npl + v;
        }
        // ---- exclusive scan of the blocks' hit counts over the workgroup ----
        const uint32_t cnt = (uint32_t)__popcll(hm);
        uint32_t inc = cnt;
        for (uint32_t d = 1; d < 64u; d <<= 1) { const uint32_t y = __shfl_up(inc, d); if (lane >= d) inc += y; }
        if (lane == 63u) s_wave[wave] = inc;
        s_hm[threadIdx.x] = hm; s_pid[threadIdx.x] = pid0;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < 4u; w++) { const uint32_t t = s_wave[w]; if (w < wave) before += t; total += t; }
        s_off[threadIdx.x] = before + inc - cnt;
        __syncthreads();
        // ---- wave w writes the entries of blocks w, w + 4, ...: lane = slot of the block ----
        for (uint32_t i = wave; i < (uint32_t)kBlock; i += 4u) {
            const unsigned long long m = s_hm[i];
            if (!m) continue;                                                             // wave-uniform
            const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
            if ((m >> lane) & 1ull) myq[qn + s_off[i] + prefix] = s_pid[i] + lane;
        }
        qn += total;
        __syncthreads();                                                                  // the tile's LDS words are free again
    }
    atomicAdd(&s_gen, generated);
    __syncthreads();
    if (threadIdx.x == 0) { qcount[blockIdx.x] = qn; gencount[blockIdx.x] = s_gen; }
}

}  // namespace rtx

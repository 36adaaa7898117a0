// rtx_k_adaptive.hpp — adaptive sampling (rtx_render_adaptive): the convergence criterion per 256-slot chunk and the compaction of the chunks still sampling into the active list
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
// The list-aware raygen / accumulate instantiations live beside their default forms (rtx_k_raygen.hpp, rtx_k_film.hpp: LIST).
#pragma once
#include "rtx_dev_common.hpp"

namespace rtx {

// THE CRITERION.  u1 holds the sum of all samples of a pixel, `half` the sum of those with an odd sample id; with an even count N the two halves are equally large and
// |even sum - odd sum| = |u1 - 2 half| estimates the noise of the sum.  float32, only + * abs max <, in exactly this order (the library is compiled without contraction):
//   d = (|a.x - (h.x + h.x)| + |a.y - (h.y + h.y)|) + |a.z - (h.z + h.z)|
//   s = (a.x + a.y) + a.z
//   converged = d * d < ((threshold * threshold) * max(s, dark_floor * N)) * N
// i.e. the relative error of the mean, |d| / N against threshold * sqrt(mean), with a floor under dark pixels.  The comparison is strict: threshold 0 converges nothing, and
// neither does a pixel without samples.  tests/test_adaptive_ref.py emulates this line for line.
__device__ __forceinline__ bool pixel_converged(const F4 a, const F4 h, float threshold, float dark_floor) {
    const float N = a.w;
    const float d = (fabsf(a.x - (h.x + h.x)) + fabsf(a.y - (h.y + h.y))) + fabsf(a.z - (h.z + h.z));
    const float s = (a.x + a.y) + a.z;
    return d * d < ((threshold * threshold) * fmaxf(s, dark_floor * N)) * N;
}

// one workgroup per local chunk of the shard, lane = slot.  A chunk converges when every valid pixel of it has; the flag is sticky (a chunk that has one is left alone):
// 0 sampling, 1 converged, 2 no valid pixel (never sampled).  Ballot per wave, one LDS word per workgroup, one plain store.
__global__ __launch_bounds__(kBlock) void k_adaptive_error(DevFrame f, const F4* __restrict__ accum, AdaptState ad, float threshold, float dark_floor) {
    __shared__ uint32_t s_bits;                      // bit 0: some valid pixel has not converged, bit 1: the chunk has a valid pixel
    uint32_t gi;
    if (!chunk_image_index(f, blockIdx.x, gi)) return;               // workgroup-uniform: padding of the shard's slot range
    if (ad.flag[gi] != 0u) return;                                   // workgroup-uniform, and nothing else writes this word during the launch
    if (threadIdx.x == 0) s_bits = 0u;
    __syncthreads();
    uint32_t x = 0, y = 0;
    const bool valid = slot_to_pixel(f, blockIdx.x * kBlock + threadIdx.x, x, y);
    bool open = false;
    if (valid) open = !pixel_converged(accum[(size_t)y * f.width + x], ad.half[(size_t)y * f.width + x], threshold, dark_floor);
    const uint32_t bits = (__ballot(open) != 0ull ? 1u : 0u) | (__ballot(valid) != 0ull ? 2u : 0u);
    if (lane_id() == 0 && bits) atomicOr(&s_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0) ad.flag[gi] = !(s_bits & 2u) ? 2u : (s_bits & 1u) ? 0u : 1u;
}

// The active list of the next pass: the local chunks that are still sampling (flag 0) and below max_spp, in ASCENDING order (neighbouring sub-queues stay on neighbouring
// pixels, timings reproduce), by a ballot / mbcnt scan in ONE workgroup — a 1080p frame has 8 100 chunks — and no global atomic.  A pass gives all its chunks the same sample ids,
// so the list holds the candidates with the LOWEST count only: within one sequence of calls on one tiling they all share it (deactivation is monotone), and chunks that came to
// different counts some other way (another sharding rendered into the same image before) catch up in passes of their own.
// out[0] list length, [1] that count, [2] chunks converged, [3] chunks sampling but at max_spp, [4] chunks with a valid pixel (known once the criterion has run).
constexpr uint32_t kCompactBlock = 1024;
__global__ __launch_bounds__(kCompactBlock) void k_adaptive_compact(DevFrame f, AdaptState ad, uint32_t max_spp, uint32_t* __restrict__ list, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_min, s_tally[3], s_wave[kCompactBlock / 64];
    const uint32_t nchunks = f.chunks_per_sample, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { s_min = 0xFFFFFFFFu; s_tally[0] = s_tally[1] = s_tally[2] = 0u; }
    __syncthreads();
    uint32_t mn = 0xFFFFFFFFu, conv = 0, atmax = 0, real = 0;
    for (uint32_t lc = threadIdx.x; lc < nchunks; lc += kCompactBlock) {
        uint32_t gi;
        if (!chunk_image_index(f, lc, gi)) continue;
        const uint32_t fl = ad.flag[gi], n = ad.count[gi];
        real += fl != 2u; conv += fl == 1u; atmax += fl == 0u && n >= max_spp;
        if (fl == 0u && n < max_spp && n < mn) mn = n;
    }
    if (mn != 0xFFFFFFFFu) atomicMin(&s_min, mn);                    // (LDS atomics; wave-level pre-reduction would save nothing at <= 8 trips)
    if (conv) atomicAdd(&s_tally[0], conv);
    if (atmax) atomicAdd(&s_tally[1], atmax);
    if (real) atomicAdd(&s_tally[2], real);
    __syncthreads();
    const uint32_t cur = s_min;
    uint32_t run = 0;                                                // entries written by the rounds before this one (uniform)
    for (uint32_t base = 0; base < nchunks; base += kCompactBlock) {
        const uint32_t lc = base + threadIdx.x;
        uint32_t gi;
        bool act = false;
        if (lc < nchunks && chunk_image_index(f, lc, gi)) act = ad.flag[gi] == 0u && ad.count[gi] == cur && cur < max_spp;
        const unsigned long long m = __ballot(act);
        const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (lane_id() == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = 0, tot = 0;
        for (uint32_t w = 0; w < kCompactBlock / 64; w++) { const uint32_t k = s_wave[w]; off += w < wave ? k : 0u; tot += k; }
        if (act) list[run + off + before] = lc;                      // run + off + before < number of candidates <= nchunks: the list holds nchunks entries
        run += tot;
        __syncthreads();                                             // s_wave is rewritten by the next round
    }
    if (threadIdx.x == 0) { out[0] = run; out[1] = run ? cur : 0u; out[2] = s_tally[0]; out[3] = s_tally[1]; out[4] = s_tally[2]; }
}

}  // namespace rtx

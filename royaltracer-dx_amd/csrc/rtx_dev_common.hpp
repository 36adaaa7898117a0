// rtx_dev_common.hpp — device-side helpers shared by all kernels: block size, wave helpers, sub-queue compaction, path slot -> pixel, primary ray
// (included by the kernel headers of rtx_kernels.hip — see its header comment for the overall design — and, for kBlock, by rtx_refit.hip)
#pragma once
#include "rtx_kernels.hpp"

namespace rtx {

constexpr int kBlock = 256;
constexpr uint32_t kMaxNee = 16;

// ---------------------------------------------------------------------------------------------
// wave-level helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// Stream compaction into a WORKGROUP-PRIVATE sub-queue: every lane of the wave must call this (convergent).
// The counter lives in LDS (one ds_add per wave); there are no global atomics anywhere in the render loop —
// a single global counter saturates at ~88 returning atomics/us on MI355X and was the first bottleneck found
// (profiles/r01_cornell_c2_v1.md).
__device__ __forceinline__ uint32_t block_push(bool pred, uint32_t* lds_counter) {
    const unsigned long long mask = __ballot(pred);
    const uint32_t cnt = (uint32_t)__popcll(mask);
    if (cnt == 0) return 0xFFFFFFFFu;                    // wave-uniform
    const uint32_t prefix = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(lds_counter, cnt);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return base + prefix;
}

// ---------------------------------------------------------------------------------------------
// pixel <-> local path-slot mapping (shard tiles, 8x8 pixel blocks inside a tile so that one wave
// covers a compact screen region)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool slot_to_pixel(const DevFrame& f, uint32_t pl, uint32_t& x, uint32_t& y) {
    const uint32_t ts2 = 2u * f.tile_shift;                  // tile_size is a power of two
    const uint32_t k = pl >> ts2, r = pl & ((1u << ts2) - 1u);
    uint32_t tx, ty;
    if (!shard_tile(f, k, tx, ty)) return false;
    const uint32_t bshift = f.tile_shift - 3u;               // 8x8 pixel blocks per tile row = 2^bshift
    const uint32_t blk = r >> 6, ln = r & 63u;
    const uint32_t bx = blk & ((1u << bshift) - 1u), by = blk >> bshift;
    x = (tx << f.tile_shift) + bx * 8u + (ln & 7u);
    y = (ty << f.tile_shift) + by * 8u + (ln >> 3);
    return x < f.width && y < f.height;
}

// rtx_render_adaptive renders a frame whose slot space is the list of active chunks (DevFrame::list): virtual slot v -> the shard's real slot.  The raygen kernels and
// k_accumulate exist in a list-aware instantiation (LIST) that passes every slot through this before slot_to_pixel and before indexing a per-real-slot table; path ids stay
// virtual (pid = sl * npl + v).  LIST = false is the identity: the default instantiations are the code they were before the parameter existed.
template <bool LIST> __device__ __forceinline__ uint32_t real_slot(const DevFrame& f, uint32_t v) {
    if constexpr (LIST) return f.list[v >> 8] * (uint32_t)kBlock + (v & 255u);
    else return v;
}
// the image chunk (tile, 256-slot strip of it) behind local chunk lc of the shard: index of its words in AdaptState; false: the shard's slot range is padded there (no tile)
__device__ __forceinline__ bool chunk_image_index(const DevFrame& f, uint32_t lc, uint32_t& gi) {
    const uint32_t cs = 2u * f.tile_shift - 8u;              // chunks per tile = 2^cs (tile_size >= 16)
    uint32_t tx, ty;
    if (!shard_tile(f, lc >> cs, tx, ty)) return false;
    gi = ((ty * f.tiles_x + tx) << cs) | (lc & ((1u << cs) - 1u));
    return true;
}

// primary ray, RayGen_v6_pass1.hlsl:51-95
__device__ __forceinline__ void primary_ray(const CameraGPU& cam, uint32_t W, uint32_t H, uint32_t x, uint32_t y, float jx, float jy, f3& o, f3& d) {
    const float dx = (((float)x + jx) / (float)W) * 2.0f - 1.0f;
    const float dy = (((float)y + jy) / (float)H) * 2.0f - 1.0f;
    const float* P = cam.projI; const float* Vi = cam.viewI;
    const float ndy = -dy;
    f3 tg = mk3(P[0] * dx + P[4] * ndy + P[8] + P[12], P[1] * dx + P[5] * ndy + P[9] + P[13], P[2] * dx + P[6] * ndy + P[10] + P[14]);
    d = normalize(xform_dir(Vi, tg));
    o = mk3(Vi[12], Vi[13], Vi[14]);
}

// the camera in LDS: every kernel that shoots primary rays copies the 64 floats once per workgroup (the caller owns the __shared__ object and the barrier)
static_assert(sizeof(CameraGPU) == 64 * sizeof(float), "stage_camera copies one float per lane of the first wave");
__device__ __forceinline__ void stage_camera(CameraGPU& cam, const CameraGPU* __restrict__ cam_p) {
    if (threadIdx.x < 64) ((float*)&cam)[threadIdx.x] = ((const float*)cam_p)[threadIdx.x];
}

// |cosine| between a primary ray and the view axis (the third column of viewI), sign-free: left- and right-handed views alike (include/rtx.h, THIN LENS: cz)
__device__ __forceinline__ float view_axis_cos(const CameraGPU& cam, f3 d) {
    const float* Vi = cam.viewI;
    return fabsf((d.x * Vi[8] + d.y * Vi[9]) + d.z * Vi[10]);
}
// PIXEL, SAMPLE -> PRIMARY RAY AND STARTING SEED of a path of rtx_render / rtx_render_adaptive: the sample's seed, RTX_FLAG_JITTER's two draws, the pinhole ray (primary_ray).
// LENS (rtx_set_lens with a radius > 0; include/rtx.h, THIN LENS, operation for operation): two more draws choose a point of the aperture disk, and the ray runs from there
// through the pinhole ray's point at view-axis depth f.lens_focus.  The path starts from the seed state after the draws.  Called by both raygen kernels and by the two debug
// probes (k_dbg_primary, k_dbg_primary_seeds); LENS = false reads neither lens member of the frame.
template <bool LENS>
__device__ __forceinline__ void camera_sample(const CameraGPU& cam, const DevFrame& f, uint32_t x, uint32_t y, uint32_t sample, f3& o, f3& d, uint32_t& s0, uint32_t& s1) {
    seed_init(x, y, sample, f.frame_seed, s0, s1);
    float jx = 0.0f, jy = 0.0f;
    if (f.flags & 2u) { jx = tea_next(s0, s1); jy = tea_next(s0, s1); }   // RayGen.hlsl:84-85
    primary_ray(cam, f.width, f.height, x, y, jx, jy, o, d);
    if constexpr (LENS) {
        const float* Vi = cam.viewI;
        const float xi1 = tea_next(s0, s1), xi2 = tea_next(s0, s1);
        const float r = sqrtf(xi1);
        float sn, cs; sincos_(kTwoPi * xi2, sn, cs);
        const float lx = (f.lens_radius * r) * cs, ly = (f.lens_radius * r) * sn;
        const float cz = view_axis_cos(cam, d);
        const float ft = f.lens_focus / cz;
        const f3 P = mk3(o.x + d.x * ft, o.y + d.y * ft, o.z + d.z * ft);                                                              // the point in focus
        const f3 ol = mk3((o.x + Vi[0] * lx) + Vi[4] * ly, (o.y + Vi[1] * lx) + Vi[5] * ly, (o.z + Vi[2] * lx) + Vi[6] * ly);          // the lens point: camera right / up
        const f3 v = mk3(P.x - ol.x, P.y - ol.y, P.z - ol.z);
        const float r2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
        const float inv = 1.0f / sqrtf(r2);
        const f3 dl = mk3(v.x * inv, v.y * inv, v.z * inv);
        if (cz > 0.0f && finite3(dl)) { o = ol; d = dl; }                  // (else the path keeps the pinhole ray; the two draws are consumed either way)
    }
}

// THE CHUNK DEAL of the raygen kernels, one row of it: a kernel walks the rows k = 0, 1, ... with `for (uint32_t k = 0, row0 = 0, c; row0 < nchunks; k++)`, nchunks =
// f.chunks_per_sample * f.batch_spp; this returns whether row k holds a chunk for this workgroup's sub-queue, and which (c), and advances row0.  Chunk c = 256 consecutive path
// slots of ONE sample; chunks are dealt round-robin to workgroups so that every workgroup's sub-queue holds a representative sample of the image (load balance across bounces).
// Even deal: chunks b, b + G, b + 2 G, ...; tapered deal (f.taper_levels > 0): row k hands chunks row0 .. row0 + n_k - 1 to the sub-queues 0 .. n_k - 1 (taper_row_width).
__device__ __forceinline__ bool dealt_chunk(const DevFrame& f, uint32_t k, uint32_t& row0, uint32_t nchunks, uint32_t& c) {
    const uint32_t nk = f.taper_levels ? taper_row_width(k, gridDim.x, f.taper_levels) : gridDim.x;
    uint32_t pos = blockIdx.x;
    if (f.taper_levels && blockIdx.x < nk) { pos += (k * 2654435761u) % nk; if (pos >= nk) pos -= nk; }      // rotate the row: every sub-queue sees every part of the image over its rows
    c = row0 + pos;
    row0 += nk;
    return !(blockIdx.x >= nk || c >= nchunks);                                           // wave-uniform
}
// The same deal without the walk: row0 of row k in closed form, for a kernel that takes its rows in parallel (k_raygen_shared) and hands the result to dealt_chunk.  The
// widths of the tapered deal repeat with period 2^(levels - 1) (taper_row_width looks at the low bits of k only); period_sum = the widths of one period.
__device__ __forceinline__ uint32_t deal_width(const DevFrame& f, uint32_t k) { return f.taper_levels ? taper_row_width(k, gridDim.x, f.taper_levels) : gridDim.x; }
__device__ __forceinline__ uint32_t deal_row0(const DevFrame& f, uint32_t k, uint32_t period, uint32_t period_sum) {
    uint32_t r = (k / period) * period_sum;
    for (uint32_t j = 0; j < (k & (period - 1u)); j++) r += deal_width(f, j);
    return r;
}

}  // namespace rtx

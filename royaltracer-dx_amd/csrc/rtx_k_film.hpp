// rtx_k_film.hpp — film kernels: accumulation, sRGB8 output, debug layers, tile slabs of the multi-GPU gather
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
#pragma once
#include "rtx_shade.hpp"

namespace rtx {

// ---------------------------------------------------------------------------------------------
// accumulate: gPermanentData running sum + count, RayGen_v6_pass3.hlsl:383-405.  Fixed order: the
// batch's samples are added in sample order, batches run in order on the stream.
// ---------------------------------------------------------------------------------------------
// LIST: the adaptive form (rtx_render_adaptive).  The frame's slots are the active list's (real_slot); beside u1 the samples with an odd id go — in the same place, in the same
// order — into `half`, the second running sum the convergence criterion compares u1 with (rtx_k_adaptive.hpp); the first lane of a chunk notes the samples the chunk has now.
// SHARED: RTX_OPT_SHARED_PRIMARY in effect — whether a pixel's paths hold a radiance is the same for all its samples: bit (slot & 63) of prim_hits[real slot >> 6]
// (k_primary_surface) in the place of the per-path p.hitmask, which that path no longer writes.
template <bool LIST, bool SHARED>
__global__ __launch_bounds__(kBlock) void k_accumulate(DevFrame f, DevPaths p, F4* __restrict__ accum, AdaptState ad, const unsigned long long* __restrict__ prim_hits) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < f.npl; pl += stride) {
        uint32_t x, y;
        if constexpr (LIST) {
            uint32_t gi;
            if ((pl & 255u) == 0u && chunk_image_index(f, f.list[pl >> 8], gi)) ad.count[gi] = ad.count[gi] + f.batch_spp;      // one lane per chunk and batch; a plain store
        }
        const uint32_t rs = real_slot<LIST>(f, pl);
        if (!slot_to_pixel(f, rs, x, y)) continue;
        bool lit = true;
        if constexpr (SHARED) lit = ((prim_hits[rs >> 6] >> (rs & 63u)) & 1ull) != 0ull;
        F4 a = accum[(size_t)y * f.width + x];
        F4 h = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (LIST) h = ad.half[(size_t)y * f.width + x];
        for (uint32_t s = 0; s < f.batch_spp; s++) {
            const size_t pid = (size_t)s * f.npl + pl;
            F4 r = {0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (SHARED) { if (lit) r = p.rad[pid]; }
            else if (!p.hitmask || ((p.hitmask[pid >> 6] >> (pl & 63u)) & 1ull)) r = p.rad[pid];
            const f3 rv = mk3(r.x, r.y, r.z);
            if (finite3(rv)) {
                a.x = a.x + rv.x; a.y = a.y + rv.y; a.z = a.z + rv.z; a.w = a.w + 1.0f;
                if constexpr (LIST) if ((f.sample_first + s) & 1u) { h.x = h.x + rv.x; h.y = h.y + rv.y; h.z = h.z + rv.z; h.w = h.w + 1.0f; }
            }
        }
        accum[(size_t)y * f.width + x] = a;
        if constexpr (LIST) ad.half[(size_t)y * f.width + x] = h;
    }
}

// sRGB8 output: RayGen_v6_pass3.hlsl:405,428-441 + Common_v6.hlsl:353-376
__global__ __launch_bounds__(kBlock) void k_srgb8(const F4* __restrict__ accum, uint32_t npix, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= npix) return;
    const F4 a = accum[i];
    const float cnt = maxf_(a.w, 1.0f);
    float c[3] = {a.x / cnt, a.y / cnt, a.z / cnt};
    if (is_nan(c[0]) || is_nan(c[1]) || is_nan(c[2])) { c[0] = 1.0f; c[1] = 0.0f; c[2] = 1.0f; }
    if (is_inf(c[0]) || is_inf(c[1]) || is_inf(c[2])) { c[0] = 0.0f; c[1] = 1.0f; c[2] = 1.0f; }
    uint32_t px = 0xFF000000u;
    for (int k = 0; k < 3; k++) {
        float v = c[k] <= 0.0031308f ? 12.92f * c[k] : 1.055f * pow_(c[k], 1.0f / 2.4f) - 0.055f;
        v = saturate(v);
        px |= ((uint32_t)(int)(v * 255.0f + 0.5f)) << (8 * k);
    }
    out[i] = px;
}

// Debug output layers (the reference's gOutput is a 30-layer texture array and 'C' cycles m_displayLevels = {0, 10..17, 20..28}: Renderer.h:298-299,
// Renderer.cpp:690-698, 748-754; its live shaders only ever write layer 0, the others show whatever was left there).  Here layers 10-17 are
// DEFINED: first-hit attributes of the pixel-corner primary ray (jitter-free, RayGen_v6_pass1.hlsl:80-95), one thread per pixel:
//   10 shading normal n/2 + 1/2   11 depth t / (1 + t)   12 material id (hashed colour)   13 Kd (fp16-rounded, as shaded; Kd' where the material has a texture map)
//   14 instance id (hashed colour)   15 barycentrics (1-u-v, u, v)   16 Ke / (1 + Ke)   17 (roughness, metallic, dissolve)
// a miss is black; layers 20-28 stay black (never written by the reference either).  Linear values, quantised like layer 0's alpha: v * 255 + 0.5.
__device__ __forceinline__ uint32_t hash_colour(uint32_t id) {
    uint32_t h = id * 2654435761u + 0x9E3779B9u; h ^= h >> 15; h *= 0x85EBCA6Bu; h ^= h >> 13;
    return 0xFF000000u | (0x404040u + (h & 0x00BFBFBFu));
}
__device__ __forceinline__ uint32_t pack_rgb8(float r, float g, float b) {
    const float c[3] = {saturate(r), saturate(g), saturate(b)};
    uint32_t px = 0xFF000000u;
    for (int k = 0; k < 3; k++) px |= ((uint32_t)(int)(c[k] * 255.0f + 0.5f)) << (8 * k);
    return px;
}
// The first hit of every pixel (debug layers, denoiser guides): the whole workgroup stages the scene's LDS, then a grid-stride loop traces the pixel-corner primary ray
// (jitter-free, kTMinCam) and hands pixel index, ray and hit record to body(i, o, d, t, u, v, prim).  Called once, by every thread of the kernel.
// CUT: the scene has a cut-out triangle: the first ACCEPTED hit (rtx_cutout.hpp)
template <bool CUT, class Body>
__device__ __forceinline__ void for_each_first_hit(const DevScene& sc, const SmallRecPair* __restrict__ small, uint32_t width, uint32_t height, const CameraGPU* __restrict__ cam, Body body) {
    extern __shared__ F4 lds[];
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < width * height; i += stride) {
        const uint32_t x = i % width, y = i / width;
        f3 o, d; primary_ray(*cam, width, height, x, y, 0.0f, 0.0f, o, d);
        float t, u, v; uint32_t prim;
        trace_ray<false, CUT>(sc, small, L, o, d, kTMinCam, kTMax, t, u, v, prim);
        body(i, o, d, t, u, v, prim);
    }
}
template <bool TEX, bool CUT = false>      // TEX: a texture map is active, layer 13 shows Kd' (rtx_texture.hpp); scenes without one run the instantiation they always ran
__global__ __launch_bounds__(kBlock) void k_debug_layer(DevScene sc, const SmallRecPair* __restrict__ small, uint32_t width, uint32_t height, const CameraGPU* __restrict__ cam, uint32_t layer, uint32_t* __restrict__ out) {
    for_each_first_hit<CUT>(sc, small, width, height, cam, [&](uint32_t i, f3 o, f3 d, float t, float u, float v, uint32_t prim) {
        uint32_t px = 0xFF000000u;
        if (prim != kMissPrim && layer >= 10u && layer <= 17u) {
            const Surf sf = surface(sc, o, d, t, u, v, prim);
            const bool hm = sf.mat < sc.nmat;
            const MatGPU& m = sc.mats[hm ? sf.mat : 0u];
            switch (layer) {
            case 10u: px = pack_rgb8(sf.normal.x * 0.5f + 0.5f, sf.normal.y * 0.5f + 0.5f, sf.normal.z * 0.5f + 0.5f); break;
            case 11u: { const float z = t / (1.0f + t); px = pack_rgb8(z, z, z); break; }
            case 12u: px = hash_colour(sf.mat); break;
            case 13u: if (TEX && hm) { const f3 kd = tex_albedo(sc, m, sf.mat, prim, u, v); px = pack_rgb8(kd.x, kd.y, kd.z); }      // (Kd' under a texture map)
                      else px = hm ? pack_rgb8(m.Kd[0], m.Kd[1], m.Kd[2]) : px;
                      break;
            case 14u: px = hash_colour(sf.inst + 0x51ED27u); break;
            case 15u: px = pack_rgb8(1.0f - u - v, u, v); break;
            case 16u: px = hm ? pack_rgb8(m.Ke[0] / (1.0f + m.Ke[0]), m.Ke[1] / (1.0f + m.Ke[1]), m.Ke[2] / (1.0f + m.Ke[2])) : px; break;
            default: px = hm ? pack_rgb8(m.Pr, m.Pm, m.alpha) : px; break;
            }
        }
        out[i] = px;
    });
}

// tile slabs for the multi-GPU gather
__global__ __launch_bounds__(kBlock) void k_pack_tiles(DevFrame f, const F4* __restrict__ accum, F4* __restrict__ slab) {
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t pl = blockIdx.x * kBlock + threadIdx.x; pl < f.npl; pl += stride) {
        uint32_t x, y;
        F4 v = {0, 0, 0, 0};
        if (slot_to_pixel(f, pl, x, y)) v = accum[(size_t)y * f.width + x];
        slab[pl] = v;
    }
}
__global__ __launch_bounds__(kBlock) void k_unpack_tiles(DevFrame f, uint32_t nshards, const F4* __restrict__ slabs, F4* __restrict__ accum) {
    const uint32_t stride = gridDim.x * kBlock;
    const uint32_t total = f.npl * nshards;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < total; i += stride) {
        DevFrame g = f; g.shard_rank = i / f.npl; g.shard_count = nshards;
        uint32_t x, y;
        if (slot_to_pixel(g, i - g.shard_rank * f.npl, x, y)) accum[(size_t)y * f.width + x] = slabs[i];
    }
}

}  // namespace rtx

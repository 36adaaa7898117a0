// rtx_texture.hpp — diffuse texture maps on the device (EXTENSION; definition: include/rtx.h, rtx_set_texture): the bilinear sampler and the per-hit albedo Kd'.
// The same functions serve k_shade<.., TEX>, debug layer 13 and the rtx_debug_texture_sample / rtx_debug_albedo probes.  float32 in exactly the written order (the library is
// built with -ffp-contract=off); tests/texture_ref.py replays it in numpy and tests/test_texture.py holds the device to it bit for bit.
// The byte -> float tables (DevScene::tex_lut, 2 x 256 floats) are read from GLOBAL memory: the index differs per lane, so the scalar cache cannot serve it, and the 2 KB stay
// in the CU's 32-KB vector L1 beside whatever else a launch reads; k_shade's LDS plan (shade_lds_plan) is left as it is for every scene (DESIGN.md, section "texture maps").
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_bsdf.hpp"
#include "rtx_cutout.hpp"

namespace rtx {

// Sample(tex, s, t): repeat wrap, OBJ's v upward (row 0 of the image is its top), bilinear over the four nearest texel centres, no mip levels (the addressing: tex_taps, rtx_cutout.hpp)
__device__ __forceinline__ f3 tex_sample(const DevScene& sc, uint32_t tex, float s, float t) {
    const TexDesc td = sc.tex_desc[tex];
    const float* T = sc.tex_lut + ((td.flags & 1u) ? 256u : 0u);
    const TexTaps P = tex_taps(sc, td, s, t);
    const float fx = P.fx, fy = P.fy;
    const uint32_t p00 = P.p00, p10 = P.p10, p01 = P.p01, p11 = P.p11;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c00 = T[(p00 >> (8 * k)) & 255u], c10 = T[(p10 >> (8 * k)) & 255u], c01 = T[(p01 >> (8 * k)) & 255u], c11 = T[(p11 >> (8 * k)) & 255u];
        const float top = c00 + fx * (c10 - c00), bot = c01 + fx * (c11 - c01);
        c[k] = top + fy * (bot - top);
    }
    return mk3(c[0], c[1], c[2]);
}

// the MaterialOptimized rounding on the device, bit for bit half_round of rtx_scene_host.cpp (also the half-precision L2 / E3 / L1 of rtx_restir.hpp)
__device__ __forceinline__ float half_round_dev(float x) {          // float -> binary16 (RNE) -> float
    const uint32_t u = f2u(x), sign = u & 0x80000000u, a = u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return x;
    if (a >= 0x477FF000u) return u2f(sign | 0x7F800000u);
    if (a < 0x33000001u) return u2f(sign);
    if (a < 0x38800000u) { const float r = rintf(u2f(a) * 16777216.0f); return u2f(sign | f2u(r * (1.0f / 16777216.0f))); }
    const uint32_t rem = a & 0x1FFFu; uint32_t base = a & ~0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (base & 0x2000u))) base += 0x2000u;
    return u2f(sign | base);
}

// Kd' of a hit on global triangle `prim` (barycentrics u, v of the hit record) whose material is `mat` = m: half_round(m.Kd * Sample(map, interpolated UV)); a material
// without a map (and every material while no map is active: sc.map_kd == nullptr) keeps m.Kd.  *tex_out: the map's texture id, or -1
__device__ __forceinline__ f3 tex_albedo(const DevScene& sc, const MatGPU& m, uint32_t mat, uint32_t prim, float u, float v, int32_t* tex_out = nullptr) {
    const int32_t tex = sc.map_kd ? sc.map_kd[mat] : -1;
    if (tex_out) *tex_out = tex;
    if (tex < 0) return mk3(m.Kd[0], m.Kd[1], m.Kd[2]);
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    const float b0 = 1.0f - u - v;
    const float s = (b0 * q[0] + u * q[2]) + v * q[4];
    const float t = (b0 * q[1] + u * q[3]) + v * q[5];
    const f3 tl = tex_sample(sc, (uint32_t)tex, s, t);
    return mk3(half_round_dev(m.Kd[0] * tl.x), half_round_dev(m.Kd[1] * tl.y), half_round_dev(m.Kd[2] * tl.z));
}
// KdPi' = Kd' / PI for the shading (the IEEE division build_materials does for the table); a material without a map keeps the table's value
__device__ __forceinline__ f3 tex_kdpi(const DevScene& sc, const MatGPU& m, uint32_t mat, uint32_t prim, float u, float v) {
    const int32_t tex = sc.map_kd[mat];
    if (tex < 0) return mk3(m.KdPi[0], m.KdPi[1], m.KdPi[2]);
    const f3 kd = tex_albedo(sc, m, mat, prim, u, v);
    return mk3(kd.x / kPI, kd.y / kPI, kd.z / kPI);
}

}  // namespace rtx

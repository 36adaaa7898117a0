// rtx_emimap.hpp — emission maps on the device (EXTENSION; definition: include/rtx.h, EMISSION MAPS): Ke' and q of a hit on an emitter whose material has RTX_MAP_KE, and the
// texel a triangle-light NEE sample multiplies the light's emission by.  The same functions serve k_shade<.., EMI> (through add_emissive and nee_sample, rtx_shade.hpp) and
// the rtx_debug_emission / rtx_debug_light_sample probes.  float32 in exactly the written order (the library is built with -ffp-contract=off); tests/emimap_ref.py replays
// it in numpy and tests/test_emimap.py holds the device to it bit for bit.  The texel fetch is tex_sample of rtx_texture.hpp: same tables, same taps, global memory.
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_texture.hpp"

namespace rtx {

// what add_emissive reads of an emissive hit under the emission maps: the radiance Ke' and the per-triangle q of the MIS pdf (nullptr there = the material's Ke and its mean)
struct EmiHit { f3 Ke; float q; };

// Ke' and q at a hit on global triangle `prim` (barycentrics u, v of the hit record) whose material `mat` = m IS an emitter (the caller's test).  Only scenes with an active
// emission map call it (sc.map_ke / emi_q != nullptr).  A material without the map keeps the table's Ke; q is the commit's table either way.  *tex_out: the map's id, or -1
__device__ __forceinline__ EmiHit emi_hit(const DevScene& sc, const MatGPU& m, uint32_t mat, uint32_t prim, float u, float v, int32_t* tex_out = nullptr) {
    EmiHit e; e.Ke = mk3(m.Ke[0], m.Ke[1], m.Ke[2]); e.q = sc.emi_q[prim];
    const int32_t tex = sc.map_ke[mat];
    if (tex_out) *tex_out = tex;
    if (tex < 0) return e;
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    const float b0 = 1.0f - u - v;
    const float s = (b0 * q[0] + u * q[2]) + v * q[4];
    const float t = (b0 * q[1] + u * q[3]) + v * q[5];
    const f3 tl = tex_sample(sc, (uint32_t)tex, s, t);
    e.Ke = mk3(half_round_dev(m.KeFull[0] * tl.x), half_round_dev(m.KeFull[1] * tl.y), half_round_dev(m.KeFull[2] * tl.z));
    return e;
}

// the texture coordinates of a light sample: u, v, w = the sample's weights of corners 0, 1, 2 (nee_sample), the corner pairs those of the light's global triangle
__device__ __forceinline__ void emi_light_uv(const DevScene& sc, uint32_t prim, float u, float v, float w, float& s, float& t) {
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    s = (u * q[0] + v * q[2]) + w * q[4];
    t = (u * q[1] + v * q[3]) + w * q[5];
}
// em * tl of a triangle-light NEE sample: the light's emission (the material's full-precision Ke) times the texel at the sampled point; a light without the map keeps em
__device__ __forceinline__ f3 emi_light_em(const DevScene& sc, const LightGPU& lt, float u, float v, float w) {
    f3 em = mk3(lt.em[0], lt.em[1], lt.em[2]);
    if (lt.emi_tex < 0) return em;
    float s, t; emi_light_uv(sc, lt.prim, u, v, w, s, t);
    const f3 tl = tex_sample(sc, (uint32_t)lt.emi_tex, s, t);
    return mk3(em.x * tl.x, em.y * tl.y, em.z * tl.z);
}

}  // namespace rtx

// rtx_specmap.hpp — specular, roughness and metalness maps on the device (EXTENSION; definition: include/rtx.h, SPECULAR MAPS): Ks', Pr', Pm' of a hit whose material has
// RTX_MAP_KS / RTX_MAP_PR / RTX_MAP_PM, and which energy table its Ess is read from.  The same functions serve k_shade<.., SPC> and the rtx_debug_specular / rtx_debug_ess
// probes.  float32 in exactly the written order (the library is built with -ffp-contract=off); tests/specmap_ref.py replays it in numpy and tests/test_specmap.py holds the
// device to it bit for bit.  The byte tables are those of DevScene::tex_lut and the energy table (rows x 16 floats, <= 16 KB) is read from global memory like them: the row
// differs per lane, and k_shade's LDS plan (shade_lds_plan) is left as it is for every scene.  The look-up itself, ess_table, stands beside ess_lut in rtx_bsdf.hpp.
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_cutout.hpp"
#include "rtx_texture.hpp"

namespace rtx {

// one byte channel (shift = 8 for green, 16 for blue) of the four taps through the LINEAR table, the same two lerps as a colour channel
__device__ __forceinline__ float spec_taps_channel(const DevScene& sc, const TexTaps& P, uint32_t shift) {
    const float* T = sc.tex_lut;
    const float c00 = T[(P.p00 >> shift) & 255u], c10 = T[(P.p10 >> shift) & 255u], c01 = T[(P.p01 >> shift) & 255u], c11 = T[(P.p11 >> shift) & 255u];
    const float top = c00 + P.fx * (c10 - c00), bot = c01 + P.fx * (c11 - c01);
    return top + P.fy * (bot - top);
}
__device__ __forceinline__ float spec_channel(const DevScene& sc, int32_t tex, float s, float t, uint32_t shift) {
    const TexDesc td = sc.tex_desc[tex];
    return spec_taps_channel(sc, tex_taps(sc, td, s, t), shift);
}

// Ks', Pr', Pm' at a hit on global triangle `prim` (barycentrics u, v of the hit record) whose material `mat` = m is NOT an emitter (the caller's test).  Only scenes with an
// active specular map call it (sc.map_ks / map_pr / map_pm != nullptr).  A slot without a map keeps the table's value.  tex_out[3]: the ks / pr / pm texture ids, or -1
__device__ __forceinline__ SpecView spec_view(const DevScene& sc, const MatGPU& m, uint32_t mat, uint32_t prim, float u, float v, int32_t* tex_out = nullptr) {
    SpecView sv; sv.Ks[0] = m.Ks[0]; sv.Ks[1] = m.Ks[1]; sv.Ks[2] = m.Ks[2]; sv.Pr = m.Pr; sv.Pm = m.Pm;
    const int32_t tks = sc.map_ks[mat], tpr = sc.map_pr[mat], tpm = sc.map_pm[mat];
    if (tex_out) { tex_out[0] = tks; tex_out[1] = tpr; tex_out[2] = tpm; }
    if ((tks & tpr & tpm) < 0) return sv;                                 // (all three are -1)
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    const float b0 = 1.0f - u - v;
    const float s = (b0 * q[0] + u * q[2]) + v * q[4];
    const float t = (b0 * q[1] + u * q[3]) + v * q[5];
    if (tks >= 0) {
        const f3 tl = tex_sample(sc, (uint32_t)tks, s, t);
        sv.Ks[0] = half_round_dev(m.Ks[0] * tl.x); sv.Ks[1] = half_round_dev(m.Ks[1] * tl.y); sv.Ks[2] = half_round_dev(m.Ks[2] * tl.z);
    }
    if (tpr >= 0 && tpm == tpr) {                                         // one packed texture in both slots: its descriptor and four taps are fetched once (the same values)
        const TexDesc td = sc.tex_desc[tpr];
        const TexTaps P = tex_taps(sc, td, s, t);
        sv.Pr = half_round_dev(m.Pr * spec_taps_channel(sc, P, 8u));
        sv.Pm = half_round_dev(m.Pm * spec_taps_channel(sc, P, 16u));
        return sv;
    }
    if (tpr >= 0) sv.Pr = half_round_dev(m.Pr * spec_channel(sc, tpr, s, t, 8u));
    if (tpm >= 0) sv.Pm = half_round_dev(m.Pm * spec_channel(sc, tpm, s, t, 16u));
    return sv;
}
// where mix_view takes the Ess of a hit on material `mat` from: the energy table while one is set and the material has a roughness map, else nullptr = m.LUT
__device__ __forceinline__ const float* spec_ess_table(const DevScene& sc, uint32_t mat) { return (sc.ess_tab && sc.map_pr[mat] >= 0) ? sc.ess_tab : nullptr; }

}  // namespace rtx

// rtx_normalmap.hpp — tangent-space normal maps on the device (EXTENSION; definition: include/rtx.h, NORMAL MAPS): the shading normal n' of a hit whose material has
// RTX_MAP_NORMAL.  The same function serves k_shade<.., NRM> and the rtx_debug_shading_normal probe.  float32 in exactly the written order, plain * + - / and sqrtf (the
// library is built with -ffp-contract=off; none of the fused helpers of rtx_math.hpp); tests/normalmap_ref.py replays it in numpy and tests/test_normalmap.py holds the
// device to it bit for bit.  The decode table Nt is the third of DevScene::tex_lut ([512, 768)), read from global memory like the other two (rtx_texture.hpp).
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_cutout.hpp"
#include "rtx_shade.hpp"

namespace rtx {

// n' at a hit on global triangle `prim` (barycentrics u, v of the hit record) whose surface() is sf and whose material sf.mat is NOT an emitter (the caller's test);
// wo = the ray's direction negated.  Only scenes with an active normal map call it (sc.tri_tan / sc.map_nrm != nullptr).  *tex_out: the map's texture id, or -1
__device__ __forceinline__ f3 nrm_perturb(const DevScene& sc, const Surf& sf, uint32_t prim, float u, float v, f3 wo, int32_t* tex_out = nullptr) {
    const f3 n = sf.normal;
    const int32_t tex = sc.map_nrm[sf.mat];
    if (tex_out) *tex_out = tex;
    if (tex < 0) return n;
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    const float b0 = 1.0f - u - v;
    const float s = (b0 * q[0] + u * q[2]) + v * q[4];
    const float t = (b0 * q[1] + u * q[3]) + v * q[5];
    const TexDesc td = sc.tex_desc[tex];
    const TexTaps P = tex_taps(sc, td, s, t);
    const float* Nt = sc.tex_lut + 512u;
    float c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float c00 = Nt[(P.p00 >> (8 * k)) & 255u], c10 = Nt[(P.p10 >> (8 * k)) & 255u], c01 = Nt[(P.p01 >> (8 * k)) & 255u], c11 = Nt[(P.p11 >> (8 * k)) & 255u];
        const float top = c00 + P.fx * (c10 - c00), bot = c01 + P.fx * (c11 - c01);
        c[k] = top + P.fy * (bot - top);
    }
    if (c[0] == 0.0f && c[1] == 0.0f) return n;                          // a flat texel changes nothing, to the bit
    const float* g = sc.tri_tan + (size_t)prim * 6u;                      // object-space T, B of the triangle
    const float* M = sc.insts[sf.inst].o2w;
    const float nn[3] = {n.x, n.y, n.z};
    float Tw[3], Bw[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        Tw[k] = (M[0 + k] * g[0] + M[4 + k] * g[1]) + M[8 + k] * g[2];
        Bw[k] = (M[0 + k] * g[3] + M[4 + k] * g[4]) + M[8 + k] * g[5];
    }
    const float dT = (nn[0] * Tw[0] + nn[1] * Tw[1]) + nn[2] * Tw[2];
    const float tv[3] = {Tw[0] - nn[0] * dT, Tw[1] - nn[1] * dT, Tw[2] - nn[2] * dT};
    const float l2 = (tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2];
    if (!(l2 > 0.0f) || l2 == INFINITY) return n;                        // no tangent (zero record: no UVs, collinear UVs), or one beyond float32
    const float inv = 1.0f / sqrtf(l2);
    const float tt[3] = {tv[0] * inv, tv[1] * inv, tv[2] * inv};
    const float bv[3] = {nn[1] * tt[2] - nn[2] * tt[1], nn[2] * tt[0] - nn[0] * tt[2], nn[0] * tt[1] - nn[1] * tt[0]};
    const float sg = ((bv[0] * Bw[0] + bv[1] * Bw[1]) + bv[2] * Bw[2]) < 0.0f ? -1.0f : 1.0f;      // handedness from the geometry: mirrored UVs and mirrored instances alike
    float m[3];
#pragma unroll
    for (int k = 0; k < 3; k++) m[k] = (tt[k] * c[0] + (bv[k] * sg) * c[1]) + nn[k] * c[2];
    const float m2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    if (!(m2 > 0.0f) || m2 == INFINITY) return n;
    const float im = 1.0f / sqrtf(m2);
    const f3 np = mk3(m[0] * im, m[1] * im, m[2] * im);
    const float a = (n.x * wo.x + n.y * wo.y) + n.z * wo.z;
    const float ap = (np.x * wo.x + np.y * wo.y) + np.z * wo.z;
    if ((a > 0.0f && !(ap > 0.0f)) || (a < 0.0f && !(ap < 0.0f))) return n;      // the map never turns the surface away from the viewer
    return np;
}

}  // namespace rtx

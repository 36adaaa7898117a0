// rtx_cutout.hpp — alpha cut-outs on the device (EXTENSION; definition: include/rtx.h, ALPHA CUT-OUTS): the texel addressing every sampler shares (tex_taps; tex_sample of
// rtx_texture.hpp reads its colour channels through it) and the alpha test a traversal runs on a geometric candidate (cut_alpha / cut_accept).
// The same functions serve traverse<.., CUT>, the persistent kernels' CUT instantiations and the rtx_debug_opacity probe.  float32 in exactly the written order (the library is
// built with -ffp-contract=off); tests/cutout_ref.py replays it in numpy and tests/test_cutout.py holds the device to it bit for bit.
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_dev_common.hpp"

namespace rtx {

__device__ __forceinline__ int tex_wrap(int i, int n) { return ((i % n) + n) % n; }

// The addressing of Sample(tex, s, t): repeat wrap, OBJ's v upward (row 0 of the image is its top), the four nearest texel centres and the two weights
struct TexTaps { uint32_t p00, p10, p01, p11; float fx, fy; };
__device__ __forceinline__ TexTaps tex_taps(const DevScene& sc, const TexDesc& td, float s, float t) {
    const int W = (int)td.width, H = (int)td.height;
    const float fs = s - floorf(s), ft = t - floorf(t);
    const float x = fs * (float)W - 0.5f, y = (1.0f - ft) * (float)H - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    TexTaps R;
    R.fx = x - x0; R.fy = y - y0;
    const int ix0 = tex_wrap((int)x0, W), ix1 = tex_wrap((int)x0 + 1, W), iy0 = tex_wrap((int)y0, H), iy1 = tex_wrap((int)y0 + 1, H);
    const uint32_t* px = sc.texels + td.offset;
    R.p00 = px[(size_t)iy0 * W + ix0]; R.p10 = px[(size_t)iy0 * W + ix1]; R.p01 = px[(size_t)iy1 * W + ix0]; R.p11 = px[(size_t)iy1 * W + ix1];
    return R;
}

// alpha of opacity texture `tex` at barycentrics (u, v) of global triangle `prim`: the interpolated UV of the map_Kd text, the alpha BYTE of the four taps through the LINEAR
// table (whatever RTX_TEX_SRGB says), the same two lerps as a colour channel
__device__ __forceinline__ float cut_alpha(const DevScene& sc, uint32_t tex, uint32_t prim, float u, float v) {
    const float* q = sc.tri_uv + (size_t)prim * 6u;
    const float b0 = 1.0f - u - v;
    const float s = (b0 * q[0] + u * q[2]) + v * q[4];
    const float t = (b0 * q[1] + u * q[3]) + v * q[5];
    const TexDesc td = sc.tex_desc[tex];
    const TexTaps P = tex_taps(sc, td, s, t);
    const float* T = sc.tex_lut;
    const float a00 = T[P.p00 >> 24], a10 = T[P.p10 >> 24], a01 = T[P.p01 >> 24], a11 = T[P.p11 >> 24];
    const float top = a00 + P.fx * (a10 - a00), bot = a01 + P.fx * (a11 - a01);
    return top + P.fy * (bot - top);
}
constexpr float kCutOff = 0.5f;                      // a candidate on a cut-out triangle counts iff its alpha >= kCutOff (fixed: no per-material cut-off)
// THE hit rule's second half: a geometric candidate on global triangle `prim` counts unless the triangle is a cut-out triangle (sc.tri_cut[prim] >= 0: its opacity texture)
// and its alpha is below the cut-off.  Only the CUT instantiations call it, and only scenes with a cut-out triangle launch those (sc.tri_cut != nullptr)
__device__ __forceinline__ bool cut_accept(const DevScene& sc, uint32_t prim, float u, float v) {
    const int32_t tex = sc.tri_cut[prim];
    if (tex < 0) return true;
    return cut_alpha(sc, (uint32_t)tex, prim, u, v) >= kCutOff;
}

}  // namespace rtx

// rtx_emimap_host.hpp — the host half of the emission maps (EXTENSION; definition: include/rtx.h, EMISSION MAPS): the sampler replayed in float32, the quadrature that
// gives a mapped emitter triangle the mean of its texels, and the weight and q of such a triangle.  rtx_commit_scene runs it (SceneHost::build_lights) for every
// emitter triangle whose material has RTX_MAP_KE, only while an emission map is active.
// Header-only and free of the library's other headers: rtx_scene_host.cpp and the stand-alone program tests/sanitize/emimap_main.cpp include it.
// float32 in exactly the written order (no contraction: written as separate statements); tests/emimap_ref.py replays it bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rtx {

constexpr int kEmiMaxSplit = 16;         // a triangle is cut into at most 16^2 sub-triangles

// byte -> float of a texel channel, as the device's table holds it (rtx_commit.hip: fill_tex_lut): linear b / 255, sRGB decoded in double and rounded once
struct EmiByteTables {
    float lin[256], srgb[256];
    EmiByteTables() {
        for (int b = 0; b < 256; b++) {
            lin[b] = (float)b / 255.0f;
            const double cs = b / 255.0;
            srgb[b] = (float)(cs <= 0.04045 ? cs / 12.92 : std::pow((cs + 0.055) / 1.055, 2.4));
        }
    }
};
inline const EmiByteTables& emi_byte_tables() { static const EmiByteTables T; return T; }

inline int emi_wrap(int i, int n) { return ((i % n) + n) % n; }

// Sample(tex, s, t) of rtx_texture.hpp / rtx_cutout.hpp on the host: the same operations on the same operands in the same order
inline void emi_sample(const uint32_t* rgba, uint32_t width, uint32_t height, bool srgb, float s, float t, float out[3]) {
    const int W = (int)width, H = (int)height;
    const float* T = srgb ? emi_byte_tables().srgb : emi_byte_tables().lin;
    const float fs = s - std::floor(s), ft = t - std::floor(t);
    const float xs = fs * (float)W, x = xs - 0.5f;
    const float yf = 1.0f - ft, ys = yf * (float)H, y = ys - 0.5f;
    const float x0 = std::floor(x), y0 = std::floor(y);
    const float fx = x - x0, fy = y - y0;
    const int ix0 = emi_wrap((int)x0, W), ix1 = emi_wrap((int)x0 + 1, W), iy0 = emi_wrap((int)y0, H), iy1 = emi_wrap((int)y0 + 1, H);
    const uint32_t p00 = rgba[(size_t)iy0 * W + ix0], p10 = rgba[(size_t)iy0 * W + ix1], p01 = rgba[(size_t)iy1 * W + ix0], p11 = rgba[(size_t)iy1 * W + ix1];
    for (int k = 0; k < 3; k++) {
        const float c00 = T[(p00 >> (8 * k)) & 255u], c10 = T[(p10 >> (8 * k)) & 255u], c01 = T[(p01 >> (8 * k)) & 255u], c11 = T[(p11 >> (8 * k)) & 255u];
        const float dt = c10 - c00, pt = fx * dt, top = c00 + pt;
        const float db = c11 - c01, pb = fx * db, bot = c01 + pb;
        const float dv = bot - top, pv = fy * dv;
        out[k] = top + pv;
    }
}

// n of the quadrature: clamp(ceil(max over the three edges of max(|du| * W, |dv| * H)), 1, 16), in double.  uv6: the corner pairs uv0, uv1, uv2
inline int emi_split(const float* uv6, uint32_t width, uint32_t height) {
    double m = 0.0;
    for (int e = 0; e < 3; e++) {
        const int a = e, b = (e + 1) % 3;
        const double du = std::fabs((double)uv6[2 * b] - (double)uv6[2 * a]) * (double)width;
        const double dv = std::fabs((double)uv6[2 * b + 1] - (double)uv6[2 * a + 1]) * (double)height;
        m = std::fmax(m, std::fmax(du, dv));
    }
    const double c = std::ceil(m);
    return !(c > 1.0) ? 1 : (c >= (double)kEmiMaxSplit ? kEmiMaxSplit : (int)c);      // (a NaN cannot come in: rtx_set_mesh_uvs refuses non-finite pairs)
}

// one centroid: hit barycentrics (u, v) rounded to float32, then b0, s, t and Sample() as at a hit
inline void emi_sample_bary(const uint32_t* rgba, uint32_t width, uint32_t height, bool srgb, const float* uv6, double ud, double vd, float out[3]) {
    const float u = (float)ud, v = (float)vd;
    const float b0a = 1.0f - u, b0 = b0a - v;
    const float s0 = b0 * uv6[0], s1 = u * uv6[2], s01 = s0 + s1, s2 = v * uv6[4], s = s01 + s2;
    const float t0 = b0 * uv6[1], t1 = u * uv6[3], t01 = t0 + t1, t2 = v * uv6[5], t = t01 + t2;
    emi_sample(rgba, width, height, srgb, s, t, out);
}

// mean[k] of the texture over the triangle: n^2 equal sub-triangles sampled at their centroids — i outer, j inner, the upright one of a cell before its inverted one —
// summed in double in that order, divided by n^2, rounded to float32 once
inline void emi_triangle_mean(const uint32_t* rgba, uint32_t width, uint32_t height, bool srgb, const float* uv6, float mean[3]) {
    const int n = emi_split(uv6, width, height);
    double sum[3] = {0.0, 0.0, 0.0};
    float tl[3];
    for (int i = 0; i < n; i++) for (int j = 0; i + j <= n - 1; j++) {
        emi_sample_bary(rgba, width, height, srgb, uv6, ((double)i + 1.0 / 3.0) / (double)n, ((double)j + 1.0 / 3.0) / (double)n, tl);
        for (int k = 0; k < 3; k++) sum[k] += (double)tl[k];
        if (i + j <= n - 2) {
            emi_sample_bary(rgba, width, height, srgb, uv6, ((double)i + 2.0 / 3.0) / (double)n, ((double)j + 2.0 / 3.0) / (double)n, tl);
            for (int k = 0; k < 3; k++) sum[k] += (double)tl[k];
        }
    }
    const double nn = (double)n * (double)n;
    for (int k = 0; k < 3; k++) mean[k] = (float)(sum[k] / nn);
}

// E[k] = KeFull[k] * mean[k] (float32); inten = (E.x + E.y + E.z) / 3: what the light scan multiplies the area by
inline float emi_intensity(const float* ke_full, const float* mean, float E[3]) {
    for (int k = 0; k < 3; k++) E[k] = ke_full[k] * mean[k];
    const float a = E[0] + E[1], b = a + E[2];
    return b / 3.0f;
}

// THE UNIT-KE RULE of the loader: a map multiplies its material's Ke, and an MTL file that names a map_Ke usually gives no Ke, which the parser records as 0: the map would
// be switched off (and the material would be no emitter).  So the step that BINDS a decoded map_Ke sets a Ke of (0, 0, 0) to (1, 1, 1).  Returns true when it changed it
inline bool emi_unit_ke(float* ke3) { if (ke3[0] == 0.0f && ke3[1] == 0.0f && ke3[2] == 0.0f) { ke3[0] = ke3[1] = ke3[2] = 1.0f; return true; } return false; }

}  // namespace rtx

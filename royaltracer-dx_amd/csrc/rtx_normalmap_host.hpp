// rtx_normalmap_host.hpp — the host half of the tangent-space normal maps (EXTENSION; definition: include/rtx.h, NORMAL MAPS): the per-triangle tangent record that
// rtx_commit_scene derives, and the two image helpers of the host layer (a height map -> a normal map, the green flip of DirectX-style maps).
// Header-only and free of the library's other headers: rtx_scene_host.cpp, host/Scenes.cpp and the stand-alone program tests/sanitize/normalmap_main.cpp include it.
// Everything is double arithmetic on float32 / byte inputs in exactly the written order, each result rounded once; tests/normalmap_ref.py replays it bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rtx {

// The tangent record of one triangle: T = dP/du (out6[0..2]) and B = dP/dv (out6[3..5]) in OBJECT space, from its corner positions p[9] and corner pairs uv[6].
// det == 0 (no UVs, collinear UVs) or a value that is not finite as a float32: six zeros.
inline void tangent_record(const float* p, const float* uv, float* out6) {
    const double e1[3] = {(double)p[3] - (double)p[0], (double)p[4] - (double)p[1], (double)p[5] - (double)p[2]};
    const double e2[3] = {(double)p[6] - (double)p[0], (double)p[7] - (double)p[1], (double)p[8] - (double)p[2]};
    const double du1 = (double)uv[2] - (double)uv[0], dv1 = (double)uv[3] - (double)uv[1], du2 = (double)uv[4] - (double)uv[0], dv2 = (double)uv[5] - (double)uv[1];
    const double det = du1 * dv2 - du2 * dv1;
    bool ok = det != 0.0;
    for (int k = 0; k < 3 && ok; k++) {
        out6[k] = (float)((e1[k] * dv2 - e2[k] * dv1) / det);
        out6[3 + k] = (float)((e2[k] * du1 - e1[k] * du2) / det);
        ok = std::isfinite(out6[k]) && std::isfinite(out6[3 + k]);
    }
    if (!ok) for (int k = 0; k < 6; k++) out6[k] = 0.0f;
}

// A height map (channel 0 of an RGBA8 image, h = byte / 255, repeat wrap, row 0 on top so that v runs upward) -> a tangent-space normal map of the same size:
// central differences scaled by `strength`, c = (-gx, -gy, 1) normalised, byte = clamp(floor(c * 127 + 128.5), 0, 255), alpha 255.
inline void HeightToNormalMap(const uint8_t* rgba, uint32_t width, uint32_t height, double strength, std::vector<uint8_t>& out) {
    out.resize((size_t)width * height * 4);
    auto h = [&](uint32_t x, uint32_t y) { return (double)rgba[((size_t)y * width + x) * 4] / 255.0; };
    for (uint32_t y = 0; y < height; y++) for (uint32_t x = 0; x < width; x++) {
        const uint32_t xm = (x + width - 1) % width, xp = (x + 1) % width, ym = (y + height - 1) % height, yp = (y + 1) % height;
        const double gx = (h(xp, y) - h(xm, y)) * 0.5 * strength;
        const double gy = (h(x, ym) - h(x, yp)) * 0.5 * strength;
        const double len = std::sqrt((gx * gx + gy * gy) + 1.0);
        const double c[3] = {-gx / len, -gy / len, 1.0 / len};
        uint8_t* o = &out[((size_t)y * width + x) * 4];
        for (int k = 0; k < 3; k++) {
            double b = std::floor(c[k] * 127.0 + 128.5);
            b = b < 0.0 ? 0.0 : (b > 255.0 ? 255.0 : b);
            o[k] = (uint8_t)b;
        }
        o[3] = 255;
    }
}

// DirectX-style maps store -bitangent in green: g' = g == 0 ? 255 : 256 - g, an exact negation under the decode table Nt (128 +- d <-> 128 -+ d; 0 and 1 both decode to -1)
inline void FlipGreen(uint8_t* rgba, size_t texels) {
    for (size_t i = 0; i < texels; i++) { const uint8_t g = rgba[i * 4 + 1]; rgba[i * 4 + 1] = g == 0 ? 255 : (uint8_t)(256 - g); }
}

}  // namespace rtx

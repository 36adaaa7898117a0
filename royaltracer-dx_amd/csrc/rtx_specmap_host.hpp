// rtx_specmap_host.hpp — the host half of the specular, roughness and metalness maps (EXTENSION; definition: include/rtx.h, SPECULAR MAPS): the validation of an energy table
// (rtx_set_ess_table), the row arithmetic of its look-up, and the zero-scalar rule of the MTL loader.
// Header-only and free of the library's other headers: rtx_scene_host.cpp, host/Scenes.cpp and the stand-alone program tests/sanitize/specmap_main.cpp include it.
// float32 in exactly the written order (no contraction: written as separate statements); tests/specmap_ref.py replays it bit for bit.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace rtx {

constexpr uint32_t kEssMinRows = 2, kEssMaxRows = 256, kEssCols = 16;

// rtx_set_ess_table's argument check: nullptr on success, else what is wrong.  (NULL, 0) clears and is valid
inline const char* ess_table_error(const float* table, uint32_t rows) {
    if (!table && !rows) return nullptr;
    if (!table) return "set_ess_table: null table with a row count";
    if (rows < kEssMinRows || rows > kEssMaxRows) return "set_ess_table: rows must be in [2, 256] (or NULL / 0 to clear)";
    for (size_t i = 0; i < (size_t)rows * kEssCols; i++) if (!std::isfinite(table[i])) return "set_ess_table: non-finite value";
    return nullptr;
}

// the two rows a roughness reads and the weight of the second: fr = pr * (rows - 1), r0 = clamp(floor(fr), 0, rows - 1), r1 = min(r0 + 1, rows - 1), wr = fr - r0
struct EssRows { uint32_t r0, r1; float wr; };
inline EssRows ess_rows_of(float pr, uint32_t rows) {
    const int last = (int)rows - 1;
    const float fr = pr * (float)last;
    const float fl = std::floor(fr);
    int r0 = !(fl > 0.0f) ? 0 : (fl >= (float)last ? last : (int)fl);             // (a NaN reads row 0, as the device's conversion does)
    const int r1 = r0 + 1 < last ? r0 + 1 : last;
    EssRows R; R.r0 = (uint32_t)r0; R.r1 = (uint32_t)r1; R.wr = fr - (float)r0;
    return R;
}
// the LUT of a material that equals a constant roughness map `pr` under the table: out16[i] = A[r0][i] + wr * (A[r1][i] - A[r0][i])
inline void ess_blend_row(const float* table, uint32_t rows, float pr, float* out16) {
    const EssRows R = ess_rows_of(pr, rows);
    const float* A0 = table + (size_t)R.r0 * kEssCols; const float* A1 = table + (size_t)R.r1 * kEssCols;
    for (uint32_t i = 0; i < kEssCols; i++) { const float d = A1[i] - A0[i]; const float s = R.wr * d; out16[i] = A0[i] + s; }
}

// THE ZERO-SCALAR RULE of the loader.  A map multiplies its material's scalar, and an MTL file that names a map usually gives no scalar, which the parser records as 0: the
// map would be switched off.  So the step that BINDS a decoded map_Pr / map_Pm / map_Ks sets a zero scalar to one.  Returns true when it changed the value (the caller then
// regenerates the material's energy LUT where Pr changed)
inline bool spec_unit_scalar(float* x) { if (*x == 0.0f) { *x = 1.0f; return true; } return false; }
inline bool spec_unit_colour(float* ks3) { if (ks3[0] == 0.0f && ks3[1] == 0.0f && ks3[2] == 0.0f) { ks3[0] = ks3[1] = ks3[2] = 1.0f; return true; } return false; }

}  // namespace rtx

// rtx_env_host.cpp — argument checks and table builder of the environment map (include/rtx.h: rtx_set_environment, TABLES).  Host only, no other header of the library.
// Everything below the float32 texels is DOUBLE, summed sequentially in row-major order, and rounded to float32 once per value: tests/env_ref.py builds the same tables
// with numpy's cumsum and tests/test_env.py compares them with what the device holds, bit for bit.
#include "rtx_env_host.hpp"
#include <math.h>
#include <string.h>

namespace rtx {

bool env_set(EnvHost& out, const float* rgb, uint32_t n, const float* m16, float scale, uint32_t flags, std::string& err) {
    if (!rgb) { err = "set_environment: null texel pointer"; return false; }
    if (n < 1 || n > 2048) { err = "set_environment: N must be in [1, 2048]"; return false; }
    if (flags & ~1u) { err = "set_environment: unknown flag bits"; return false; }
    if (!(scale >= 0.0f) || !isfinite(scale)) { err = "set_environment: scale must be finite and >= 0"; return false; }
    float rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (m16) {
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) rot[r * 3 + c] = m16[c * 4 + r];
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) {             // columns orthonormal: (R^T R)[a][b] = delta within 1e-4
            double s = 0.0;
            for (int r = 0; r < 3; r++) s += (double)rot[r * 3 + a] * (double)rot[r * 3 + b];
            if (!(fabs(s - (a == b ? 1.0 : 0.0)) <= 1e-4)) { err = "set_environment: env_to_world's upper 3x3 is not orthonormal within 1e-4"; return false; }
        }
    }
    const size_t cnt = (size_t)n * n * 3;
    for (size_t k = 0; k < cnt; k++) if (!(rgb[k] >= 0.0f) || !isfinite(rgb[k])) { err = "set_environment: a texel component is negative or not finite"; return false; }
    std::vector<float> scaled(cnt);
    for (size_t k = 0; k < cnt; k++) {
        scaled[k] = rgb[k] * scale;
        if (!isfinite(scaled[k])) { err = "set_environment: texel * scale is not finite"; return false; }
    }
    out.n = n; out.flags = flags; memcpy(out.rot, rot, sizeof(rot)); out.rgb.swap(scaled);
    return true;
}

double env_centre_r3(uint32_t i, uint32_t j, uint32_t n) {
    const double u = ((double)i + 0.5) / (double)n, v = ((double)j + 0.5) / (double)n;
    double a = 2.0 * u - 1.0, b = 2.0 * v - 1.0;
    const double y = (1.0 - fabs(a)) - fabs(b);
    if (y < 0.0) {
        const double fa = (1.0 - fabs(b)) * (a >= 0.0 ? 1.0 : -1.0), fb = (1.0 - fabs(a)) * (b >= 0.0 ? 1.0 : -1.0);
        a = fa; b = fb;
    }
    const double r2 = (a * a + y * y) + b * b;
    return r2 * sqrt(r2);
}

void env_build_tables(const EnvHost& e, EnvTables& t) {
    const uint32_t n = e.n; const size_t nn = (size_t)n * n;
    std::vector<double> w(nn);
    double total = 0.0;
    for (uint32_t j = 0; j < n; j++) for (uint32_t i = 0; i < n; i++) {
        const float* px = &e.rgb[((size_t)j * n + i) * 3];
        const double wt = ((((double)px[0] + (double)px[1]) + (double)px[2]) / 3.0) / env_centre_r3(i, j, n);
        w[(size_t)j * n + i] = wt;
        total += wt;
    }
    t.total = total;
    t.texels4.assign(nn * 4, 0.0f); t.marginal.assign(n, 2.0f); t.conditional.assign(nn, 2.0f);
    for (size_t k = 0; k < nn; k++) {
        t.texels4[k * 4] = e.rgb[k * 3]; t.texels4[k * 4 + 1] = e.rgb[k * 3 + 1]; t.texels4[k * 4 + 2] = e.rgb[k * 3 + 2];
        t.texels4[k * 4 + 3] = total > 0.0 ? (float)(w[k] / total) : 0.0f;
    }
    if (!(total > 0.0)) return;                               // no mass: every CDF entry stays 2.0f, and nothing samples them
    double acc = 0.0; int64_t last_row = -1;
    for (uint32_t j = 0; j < n; j++) {
        double racc = 0.0; int64_t last = -1;
        for (uint32_t i = 0; i < n; i++) { racc += w[(size_t)j * n + i]; if (w[(size_t)j * n + i] > 0.0) last = i; }
        const double rsum = racc;
        acc += rsum;                                          // (the row's own sequential sum, added to the running one)
        if (last >= 0) {
            last_row = j;
            racc = 0.0;
            for (uint32_t i = 0; i < n; i++) { racc += w[(size_t)j * n + i]; if ((int64_t)i < last) t.conditional[(size_t)j * n + i] = (float)(racc / rsum); }
        }
        t.marginal[j] = (float)(acc / total);
    }
    for (uint32_t j = 0; j < n; j++) if ((int64_t)j >= last_row) t.marginal[j] = 2.0f;
}

}  // namespace rtx

// env_main.cpp — stand-alone driver of the environment's host code for the sanitizers (tests/test_env_ref.py compiles it with csrc/rtx_env_host.cpp and host/ImageIO.cpp
// under -fsanitize=address,undefined and runs it as a child process): the argument checks and the table builder on maps with and without mass, both high-dynamic-range
// readers and the latitude-longitude conversion on every file named on the command line — the good ones and the truncated / corrupt ones alike.
// usage: env_main FILE...     prints one line per file ("ok W H" / "refused: why") and "done"
#include <cmath>
#include <cstdio>
#include <string>
#include <vector>
#include "rtx_env_host.hpp"
#include "ImageIO.h"

static int fail(const char* what) { printf("FAILED: %s\n", what); return 1; }

static int tables_of(const std::vector<float>& rgb, uint32_t n, const float* m16, float scale, bool expect_mass) {
    rtx::EnvHost e; std::string err;
    if (!rtx::env_set(e, rgb.data(), n, m16, scale, 0, err)) return fail(err.c_str());
    rtx::EnvTables t; rtx::env_build_tables(e, t);
    if (t.texels4.size() != (size_t)n * n * 4 || t.marginal.size() != n || t.conditional.size() != (size_t)n * n) return fail("table sizes");
    if ((t.total > 0.0) != expect_mass) return fail("total weight");
    double pmf = 0.0;
    for (size_t k = 0; k < (size_t)n * n; k++) pmf += t.texels4[k * 4 + 3];
    if (expect_mass && std::fabs(pmf - 1.0) > 1e-4) return fail("pmf does not sum to 1");
    if (t.marginal[n - 1] != 2.0f) return fail("the marginal CDF does not end in 2.0f");
    for (uint32_t j = 0; j < n; j++) if (t.conditional[(size_t)j * n + n - 1] != 2.0f) return fail("a conditional CDF does not end in 2.0f");
    return 0;
}

int main(int argc, char** argv) {
    // ---- the builder ----
    uint32_t seed = 12345u;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8) * (1.0f / 16777216.0f); };
    for (uint32_t n : {1u, 2u, 8u, 37u, 64u}) {
        std::vector<float> rgb((size_t)n * n * 3);
        for (float& v : rgb) v = rnd() < 0.3f ? 0.0f : rnd() * 10.0f;
        if (n == 1) rgb = {1.0f, 1.0f, 1.0f};
        if (tables_of(rgb, n, nullptr, 1.0f, true)) return 1;
        if (tables_of(rgb, n, nullptr, 0.0f, false)) return 1;                       // scale 0: no mass, every CDF entry 2.0f
        std::vector<float> sun((size_t)n * n * 3, 0.0f);
        sun[((size_t)(n / 2) * n + n / 3) * 3] = 1000.0f;                            // one texel
        if (tables_of(sun, n, nullptr, 2.0f, true)) return 1;
    }
    {   // the refusals leave the environment as it was
        rtx::EnvHost e; std::string err; std::vector<float> one = {1.0f, 2.0f, 3.0f};
        if (!rtx::env_set(e, one.data(), 1, nullptr, 1.0f, 1u, err)) return fail("a valid call was refused");
        const float skew[16] = {1, 0, 0, 0, 0.5f, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
        std::vector<float> neg = {1.0f, -1.0f, 3.0f}, nan = {1.0f, NAN, 3.0f}, big = {3e38f, 0.0f, 0.0f};
        if (rtx::env_set(e, nullptr, 1, nullptr, 1.0f, 0, err) || rtx::env_set(e, one.data(), 0, nullptr, 1.0f, 0, err) || rtx::env_set(e, one.data(), 2049, nullptr, 1.0f, 0, err) ||
            rtx::env_set(e, one.data(), 1, skew, 1.0f, 0, err) || rtx::env_set(e, one.data(), 1, nullptr, -1.0f, 0, err) || rtx::env_set(e, one.data(), 1, nullptr, INFINITY, 0, err) ||
            rtx::env_set(e, one.data(), 1, nullptr, 1.0f, 2u, err) || rtx::env_set(e, neg.data(), 1, nullptr, 1.0f, 0, err) || rtx::env_set(e, nan.data(), 1, nullptr, 1.0f, 0, err) ||
            rtx::env_set(e, big.data(), 1, nullptr, 4.0f, 0, err)) return fail("an invalid call was accepted");
        if (e.n != 1 || e.flags != 1u || e.rgb != one) return fail("a refused call changed the environment");
    }
    // ---- the readers and the conversion ----
    for (int i = 1; i < argc; i++) {
        std::vector<float> px; uint32_t w = 0, h = 0; std::string err;
        if (!ReadHDRImage(argv[i], px, w, h, err)) { printf("refused: %s\n", err.c_str()); continue; }
        if (px.size() != (size_t)w * h * 3) return fail("reader returned another size than it reports");
        for (uint32_t n : {1u, 5u, 16u}) {
            std::vector<float> oct((size_t)n * n * 3);
            if (!LatLongToOctahedral(px.data(), w, h, n, oct.data())) return fail("conversion refused a valid image");
        }
        printf("ok %u %u\n", w, h);
    }
    if (LatLongToOctahedral(nullptr, 4, 2, 4, nullptr)) return fail("conversion accepted null arrays");
    printf("done\n");
    return 0;
}

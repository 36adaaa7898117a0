// rtx_env_host.hpp — the environment map on the host (definition: include/rtx.h, rtx_set_environment): argument checks and the commit-time table builder.
// HOST ONLY and free of every other header of the library, so that rtx_env_host.cpp compiles stand-alone (tests/sanitize/env_main.cpp runs it under the sanitizers).
#pragma once
#include <stdint.h>
#include <string>
#include <vector>

namespace rtx {

// what rtx_set_environment keeps: the N x N texels with the scale multiplied in (float32, once), the rotation as rot[r * 3 + c] (row r, column c of env_to_world's upper 3x3)
struct EnvHost {
    uint32_t n = 0, flags = 0;                  // n == 0: no environment bound
    float rot[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<float> rgb;                     // n * n * 3, row-major (row j = v, column i = u)
};
// what the device holds: (r, g, b, pmf) per texel, the marginal CDF over the rows, the conditional CDF of every row; total = the sum of the weights (0: no NEE slot)
struct EnvTables { std::vector<float> texels4, marginal, conditional; double total = 0.0; };

// the checks of rtx_set_environment; on failure `out` is untouched and err says why.  m16 may be NULL (identity)
bool env_set(EnvHost& out, const float* rgb32f, uint32_t n, const float* m16, float scale, uint32_t flags, std::string& err);
// rc^3 of the texel centre (i + 0.5, j + 0.5) / N, in double: the inverse fold of the header, r2 * sqrt(r2)
double env_centre_r3(uint32_t i, uint32_t j, uint32_t n);
void env_build_tables(const EnvHost& e, EnvTables& t);

}  // namespace rtx

// rtx_env.hpp — environment lighting on the device (EXTENSION; definition: include/rtx.h, rtx_set_environment): the octahedral mapping both ways, the NEAREST lookup and the
// importance sampler.  The same functions serve k_shade<.., ENV> (miss branch, environment NEE slot) and the rtx_debug_env_* probes.  float32 in exactly the written order
// (the library is built with -ffp-contract=off; the fused dot() of rtx_math.hpp is NOT used here); tests/env_ref.py replays it in numpy and tests/test_env.py holds the device
// to it bit for bit.  No transcendental function: |x|, + - * /, sqrtf, comparisons.
#pragma once
#include "rtx_kernels.hpp"
#include "rtx_math.hpp"

namespace rtx {

__device__ __forceinline__ float env_sgn(float x) { return x >= 0.0f ? 1.0f : -1.0f; }         // sgn(-0.0f) = 1
// e = R^T d (world -> environment frame) and w = R q (environment frame -> world); rot[r * 3 + c] = row r, column c of env_to_world's upper 3x3
__device__ __forceinline__ f3 env_from_world(const DevScene& sc, f3 d) {
    const float* R = sc.env_rot;
    return mk3((R[0] * d.x + R[3] * d.y) + R[6] * d.z, (R[1] * d.x + R[4] * d.y) + R[7] * d.z, (R[2] * d.x + R[5] * d.y) + R[8] * d.z);
}
__device__ __forceinline__ f3 env_to_world(const DevScene& sc, f3 q) {
    const float* R = sc.env_rot;
    return mk3((R[0] * q.x + R[1] * q.y) + R[2] * q.z, (R[3] * q.x + R[4] * q.y) + R[5] * q.z, (R[6] * q.x + R[7] * q.y) + R[8] * q.z);
}

// direction -> map: texel (column i, row j) as j * N + i, and r3 = |q|^3 of the direction's point q on the L1 unit sphere
__device__ __forceinline__ uint32_t env_encode(const DevScene& sc, f3 d, float& r3) {
    const f3 e = env_from_world(sc, d);
    const float s = (fabsf(e.x) + fabsf(e.y)) + fabsf(e.z);
    const f3 q = mk3(e.x / s, e.y / s, e.z / s);
    float a = q.x, b = q.z;
    if (!(q.y >= 0.0f)) { a = (1.0f - fabsf(q.z)) * env_sgn(q.x); b = (1.0f - fabsf(q.x)) * env_sgn(q.z); }
    const float u = a * 0.5f + 0.5f, v = b * 0.5f + 0.5f;
    const int N = (int)sc.env_n;
    // (a direction that is not finite gives no defined texel; the lower clamp only keeps such a lane's read inside the table)
    const int i = min(max((int)(u * (float)N), 0), N - 1), j = min(max((int)(v * (float)N), 0), N - 1);
    const float r2 = (q.x * q.x + q.y * q.y) + q.z * q.z;
    r3 = r2 * sqrtf(r2);
    return (uint32_t)j * (uint32_t)N + (uint32_t)i;
}
// map -> direction in the ENVIRONMENT frame (unit length); r3 as above, of the same point
__device__ __forceinline__ f3 env_decode(float u, float v, float& r3) {
    float a = u * 2.0f - 1.0f, b = v * 2.0f - 1.0f;
    const float y = (1.0f - fabsf(a)) - fabsf(b);
    if (y < 0.0f) { const float fa = (1.0f - fabsf(b)) * env_sgn(a), fb = (1.0f - fabsf(a)) * env_sgn(b); a = fa; b = fb; }
    const float r2 = (a * a + y * y) + b * b;
    const float sr = sqrtf(r2);
    r3 = r2 * sr;
    const float inv = 1.0f / sr;
    return mk3(a * inv, y * inv, b * inv);
}
// solid-angle pdf of a direction in a texel of probability pmf
__device__ __forceinline__ float env_pdf(const DevScene& sc, float pmf, float r3) { return ((pmf * (float)(sc.env_n * sc.env_n)) * 0.25f) * r3; }

// L(d) and pdf(d): one 16-byte read
struct EnvEval { f3 L; float pdf, r3; uint32_t texel; };
__device__ __forceinline__ EnvEval env_eval(const DevScene& sc, f3 d) {
    EnvEval E;
    E.texel = env_encode(sc, d, E.r3);
    const F4 t = sc.env_tex[E.texel];
    E.L = mk3(t.x, t.y, t.z);
    E.pdf = env_pdf(sc, t.w, E.r3);
    return E;
}

// first index in [0, n) with xi < C[index] (the light CDF's search of nee_sample); the 2.0f entries at the end of every table end it for xi = 1.0f
__device__ __forceinline__ uint32_t env_search(const float* __restrict__ C, uint32_t n, float xi) {
    int left = 0, right = (int)n - 1, sel = 0;
    while (left <= right) {
        const int mid = left + (right - left) / 2;
        if (xi < C[mid]) { sel = mid; right = mid - 1; } else left = mid + 1;
    }
    return (uint32_t)sel;
}
// one environment sample: four draws — row, column, u offset, v offset.  marg: the marginal CDF (global memory, or the copy k_shade staged in LDS).  Ln = world direction;
// L and the pmf are the CHOSEN texel's, r3 the decoded point's.
__device__ __forceinline__ EnvEval env_sample(const DevScene& sc, const float* __restrict__ marg, uint32_t& s0, uint32_t& s1, f3& Ln) {
    const uint32_t N = sc.env_n;
    const float xr = tea_next(s0, s1), xc = tea_next(s0, s1), xu = tea_next(s0, s1), xv = tea_next(s0, s1);
    const uint32_t j = env_search(marg, N, xr);
    const uint32_t i = env_search(sc.env_cond + (size_t)j * N, N, xc);
    const float u = ((float)i + xu) / (float)N, v = ((float)j + xv) / (float)N;
    EnvEval E;
    Ln = env_to_world(sc, env_decode(u, v, E.r3));
    E.texel = j * N + i;
    const F4 t = sc.env_tex[E.texel];
    E.L = mk3(t.x, t.y, t.z);
    E.pdf = env_pdf(sc, t.w, E.r3);
    return E;
}

}  // namespace rtx

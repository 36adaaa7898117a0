// rtx_k_denoise.hpp — rtx_denoise and rtx_denoise_variance: the edge-avoiding a-trous filters guided by first-hit geometry (definition: include/rtx.h; host side: rtx_denoise.hip)
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
//
// PARITY-CRITICAL: tests/test_denoise_ref.py replays dn_tap operation for operation in numpy float32.  Only + - * / abs max, in the written order; no dot() / madd3() here
// (those are fused), and the tap sum is sequential in tap order.  Do not reassociate, do not split the 5 x 5 window into passes.
//
// ONE guides body (dn_guides) and ONE level body (dn_level); everything a call can choose is a template argument of theirs.  MAPS / FL: the two opt-in guide extensions
// (RTX_DENOISE_ALBEDO, RTX_DENOISE_MAPPED_NORMALS; rtx.h, MAP GUIDES) — a call with flags == 0 runs forms that never read the map-guide record; twin: tests/denoise_maps_ref.py.
// VAR: rtx_denoise_variance, which differs from rtx_denoise in what a colour record carries in w, in the colour stop and in a 3 x 3 prefilter; twin: tests/denoise_var_ref.py.
#pragma once
#include "rtx_k_film.hpp"
#include "rtx_texture.hpp"
#include "rtx_normalmap.hpp"

namespace rtx {

constexpr uint32_t kDnNoGeo = 0xFFFFFFFFu;          // material word of a guide record: the pixel is not filterable by geometry (miss, material out of range, emitter seen directly)
constexpr uint32_t kDnAlbedo = 1u, kDnMappedNormals = 2u;   // RTX_DENOISE_ALBEDO, RTX_DENOISE_MAPPED_NORMALS
constexpr float kDnAlbedoFloor = 0.015625f;             // 2^-6: part of the definition of A
constexpr uint32_t kDnTileW = 32, kDnTileH = 8;     // one workgroup = 32 x 8 pixels: a wave is two rows of 32 neighbouring pixels, 512 contiguous bytes of a colour row each

// Guides: the first hit of every pixel (for_each_first_hit, as k_debug_layer) and surface(); two F4 per pixel: (P, material word) (n, 0).  A pixel that is not filterable by geometry
// gets (0, 0, 0, kDnNoGeo) (0, 0, 0, 0), so that a tap's class test and its material test are ONE compare of the material word with the centre's.
// MAPS: also the map-guide record, two F4 per pixel: (A, 0) (nm, 0) — A = max(Kd', 2^-6) per channel (tex_albedo), nm = the normal-mapped shading normal (nrm_perturb, wo = -d);
// (1, 1, 1, 0) (0, 0, 0, 0) for a pixel that is not filterable by geometry.  sc.map_kd, sc.map_nrm and sc.tri_tan are null while no such map is active: A = max(m.Kd, 2^-6), nm = n
template <bool CUT, bool MAPS>
__device__ __forceinline__ void dn_guides(const DevScene& sc, const SmallRecPair* __restrict__ small, uint32_t width, uint32_t height, const CameraGPU* __restrict__ cam, F4* __restrict__ guides, F4* __restrict__ mguides) {
    for_each_first_hit<CUT>(sc, small, width, height, cam, [&](uint32_t i, f3 o, f3 d, float t, float u, float v, uint32_t prim) {
        F4 g0 = {0.0f, 0.0f, 0.0f, u2f(kDnNoGeo)}, g1 = {0.0f, 0.0f, 0.0f, 0.0f};
        F4 m0 = {1.0f, 1.0f, 1.0f, 0.0f}, m1 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (prim != kMissPrim) {
            const Surf sf = surface(sc, o, d, t, u, v, prim);
            if (sf.mat < sc.nmat) {
                const MatGPU& m = sc.mats[sf.mat];
                if (!(m.KeFull[0] > 0.0f || m.KeFull[1] > 0.0f || m.KeFull[2] > 0.0f)) {
                    g0 = {sf.pos.x, sf.pos.y, sf.pos.z, u2f(sf.mat)};
                    g1 = {sf.normal.x, sf.normal.y, sf.normal.z, 0.0f};
                    if constexpr (MAPS) {
                        const f3 K = tex_albedo(sc, m, sf.mat, prim, u, v);
                        m0 = {maxf_(K.x, kDnAlbedoFloor), maxf_(K.y, kDnAlbedoFloor), maxf_(K.z, kDnAlbedoFloor), 0.0f};
                        f3 nm = sf.normal;
                        if (sc.tri_tan && sc.map_nrm && !(m.Ke_len > 0.0f)) nm = nrm_perturb(sc, sf, prim, u, v, -d);
                        m1 = {nm.x, nm.y, nm.z, 0.0f};
                    }
                }
            }
        }
        guides[2 * (size_t)i] = g0; guides[2 * (size_t)i + 1] = g1;
        if constexpr (MAPS) { mguides[2 * (size_t)i] = m0; mguides[2 * (size_t)i + 1] = m1; }
    });
}
template <bool CUT, bool MAPS>
__global__ __launch_bounds__(kBlock) void k_denoise_guides(DevScene sc, const SmallRecPair* __restrict__ small, uint32_t width, uint32_t height, const CameraGPU* __restrict__ cam, F4* __restrict__ guides, F4* __restrict__ mguides) {
    dn_guides<CUT, MAPS>(sc, small, width, height, cam, guides, mguides);
}

// A colour record is (c.xyz, w).  rtx_denoise: w marks "the pixel holds samples" (1, else 0).  rtx_denoise_variance (VAR): w is v, the VARIANCE of the mean's luminance, between
// levels and in LDS, so both filters stage the same bytes per pixel.  v is never negative (a square, or a sum of products of squares; it may be +inf or NaN), so "the pixel holds
// no samples" is w = -1: a record counts for a tap while !(w < 0).
constexpr float kDnvNoSamples = -1.0f;
constexpr float kDnvEps = 9.5367431640625e-07f;      // 2^-20: part of the definition of inv
__device__ __forceinline__ float dnv_luma(float x, float y, float z) { return (0.2126f * x + 0.7152f * y) + 0.0722f * z; }
template <bool VAR> __device__ __forceinline__ bool dn_sampled(F4 c) { if constexpr (VAR) return !(c.w < 0.0f); else return c.w != 0.0f; }

// RTX_DENOISE_ALBEDO, level 0: the input colour of a FILTERABLE pixel is its mean divided by A, channel by channel (the second of the two IEEE divisions of rtx.h)
__device__ __forceinline__ void dn_demodulate(F4& c, F4 A) { c.x = c.x / A.x; c.y = c.y / A.y; c.z = c.z / A.z; }

// the record a level reads.  Level 0 (FIRST) reads u1 and forms the mean as k_srgb8 does, c = u1.xyz / max(u1.w, 1); under kDnAlbedo a pixel that holds samples and is filterable
// by geometry (geo) has it divided by A.  VAR: also e = (u1.xyz - (hb.xyz + hb.xyz)) / cnt from `half`, divided by A alike, and v = luma(e)^2.
// Every later level reads the previous one's output as it is, which carries w on
template <bool FIRST, bool ALB, bool VAR> __device__ __forceinline__ F4 dn_record(const F4* __restrict__ in, const F4* __restrict__ half, const F4* __restrict__ mg, size_t q, bool geo) {
    const F4 a = in[q];
    if constexpr (!FIRST) return a;
    else {
        const float cnt = maxf_(a.w, 1.0f);
        F4 c = {a.x / cnt, a.y / cnt, a.z / cnt, VAR ? kDnvNoSamples : 0.0f};
        if (!(a.w > 0.0f)) return c;
        if constexpr (!VAR) {
            c.w = 1.0f;
            if constexpr (ALB) { if (geo) dn_demodulate(c, mg[2 * q]); }
        } else {
            const F4 hb = half[q];
            float ex = (a.x - (hb.x + hb.x)) / cnt, ey = (a.y - (hb.y + hb.y)) / cnt, ez = (a.z - (hb.z + hb.z)) / cnt;
            if constexpr (ALB) { if (geo) { const F4 A = mg[2 * q]; dn_demodulate(c, A); ex = ex / A.x; ey = ey / A.y; ez = ez / A.z; } }
            const float el = dnv_luma(ex, ey, ez);
            c.w = el * el;
        }
        return c;
    }
}

// VAR: 1 / (sigma_var * sqrt(gv) + 2^-20) from the prefilter's two sums
__device__ __forceinline__ float dnv_inv(float sg, float sgw, float sigma_var) { const float gv = sg / sgw; return 1.0f / (sigma_var * sqrtf(gv) + kDnvEps); }
__device__ __forceinline__ float dnv_g(int dy, int dx) { return (dy == 0 ? 0.5f : 0.25f) * (dx == 0 ? 0.5f : 0.25f); }      // (1/16, 1/8, 1/16, 1/8, 1/4, 1/8, 1/16, 1/8, 1/16)

// one tap that counts (inside the image, filterable, the centre's material): rtx.h's eight lines.  np / nq: the normals of the normal stop — g1p / g1q, or the map guides' nm
// under RTX_DENOISE_MAPPED_NORMALS; the plane stop keeps g1p either way.  The colour stop is 1 - distance * inv: the L1 distance of the colours with inv = a.inv_sigma_color_s,
// or (VAR) the distance of the luminances (lum: the centre's) with inv = dnv_inv of the centre, and S.v sums the variances (dead otherwise)
struct DnSum { float x, y, z, w, v; };
template <bool VAR>
__device__ __forceinline__ void dn_tap(DnSum& S, const DenoiseLevel& a, F4 g0p, F4 g1p, F4 np, F4 cp, float lum, float inv, F4 g0q, F4 nq, F4 cq, float hh) {
    const float dn = (np.x * nq.x + np.y * nq.y) + np.z * nq.z;
    float wn = maxf_(dn, 0.0f);
    for (uint32_t k = 0; k < a.normal_power_log2; k++) wn = wn * wn;
    const float dx = g0q.x - g0p.x, dy = g0q.y - g0p.y, dz = g0q.z - g0p.z;
    const float dp = fabsf((g1p.x * dx + g1p.y * dy) + g1p.z * dz);
    const float wp = maxf_(1.0f - dp * a.inv_sigma_plane, 0.0f);
    float dc;
    if constexpr (VAR) dc = fabsf(dnv_luma(cq.x, cq.y, cq.z) - lum);
    else dc = (fabsf(cq.x - cp.x) + fabsf(cq.y - cp.y)) + fabsf(cq.z - cp.z);
    const float wc = maxf_(1.0f - dc * inv, 0.0f);
    const float w = (hh * wn) * (wp * wc);
    S.x = S.x + w * cq.x; S.y = S.y + w * cq.y; S.z = S.z + w * cq.z; S.w = S.w + w;
    if constexpr (VAR) S.v = S.v + (w * w) * cq.w;
}
__device__ __forceinline__ float dn_h(int k) { return k == 0 ? 0.375f : ((k == 1 || k == -1) ? 0.25f : 0.0625f); }      // (1/16, 1/4, 3/8, 1/4, 1/16): every product of two is exact

// One level, one thread per pixel.  S = 0: DIRECT — every tap is a global load; the lanes of a wave read neighbouring addresses at every tap (the offset is the same for
// all), so the loads coalesce and the 25-fold reuse is the cache's.  S = 1, 2, 4: STAGED — the tile plus its 2 S halo (colour and both guide records, 48 B per pixel) goes
// through LDS once, pixels outside the image as kDnNoGeo; S is the level's step and must equal a.step.  No atomics, no dependency between workgroups.
// FIRST also counts the filterable pixels of the tile into partial[workgroup] (k_denoise_count sums them).
// FL, the flags word at compile time (0: mg is never read).  kDnAlbedo: level 0 divides the colour of a filterable pixel by A where it LOADS it (at staging, or per tap in the
// direct form) and the last level multiplies the centre's result by A where it STORES it — A never enters LDS, and a pass-through pixel is neither divided nor multiplied.
// kDnMappedNormals: nm is the normal of the normal stop; the staged forms carry it as a fourth F4 per pixel (64 B per pixel, 72 KiB at step 4: two workgroups per CU, as at 54 KiB).
// VAR: sigma_var and (FIRST) half are read, a.inv_sigma_color_s is not.  The prefilter's nine positions lie ONE pixel apart whatever the step: the staged forms read them from
// the tile (the halo 2 S >= 2 covers them), the direct form from global memory.
// DBG (rtx_debug_denoise_variance): the kernel stores (v, gv) of the centre into dbg, (0, 0) for a pixel that is not filterable, and nothing else.
template <uint32_t S, bool FIRST, uint32_t FL, bool VAR, bool DBG = false>
__device__ __forceinline__ void dn_level(const DenoiseLevel& a, float sigma_var, const F4* __restrict__ in, const F4* __restrict__ half, const F4* __restrict__ guides, const F4* __restrict__ mg, F4* __restrict__ out, uint32_t* __restrict__ partial, float* __restrict__ dbg) {
    static_assert(FL <= 3u, "the flags word");
    static_assert(!DBG || (VAR && FIRST && S == 0), "the debug form is the direct first level of the variance-guided filter");
    constexpr bool ALB = (FL & kDnAlbedo) != 0, NM = (FL & kDnMappedNormals) != 0;
    constexpr uint32_t RW = kDnTileW + 4u * S, RH = kDnTileH + 4u * S;
    __shared__ F4 s_c[S ? RW * RH : 1], s_g0[S ? RW * RH : 1], s_g1[S ? RW * RH : 1], s_nm[S && NM ? RW * RH : 1];
    __shared__ uint32_t s_cnt[kBlock / 64];
    const uint32_t tx = blockIdx.x % a.tiles_x, ty = blockIdx.x / a.tiles_x;
    const uint32_t lx = threadIdx.x & (kDnTileW - 1u), ly = threadIdx.x / kDnTileW;
    const int x0 = (int)(tx * kDnTileW), y0 = (int)(ty * kDnTileH), W = (int)a.width, H = (int)a.height;
    const int x = x0 + (int)lx, y = y0 + (int)ly, s = (int)a.step;
    if constexpr (S != 0) {
        for (uint32_t i = threadIdx.x; i < RW * RH; i += kBlock) {
            const int qx = x0 - 2 * (int)S + (int)(i % RW), qy = y0 - 2 * (int)S + (int)(i / RW);
            // a position outside the image reads its nearest pixel (always in bounds, no divergent load) and is marked kDnNoGeo: it counts for no tap
            const bool ins = qx >= 0 && qx < W && qy >= 0 && qy < H;
            const size_t q = (size_t)(qy < 0 ? 0 : (qy >= H ? H - 1 : qy)) * a.width + (size_t)(qx < 0 ? 0 : (qx >= W ? W - 1 : qx));
            F4 g0 = guides[2 * q]; const F4 g1 = guides[2 * q + 1];
            const F4 c = dn_record<FIRST, ALB, VAR>(in, half, mg, q, f2u(g0.w) != kDnNoGeo);
            if (!ins) g0.w = u2f(kDnNoGeo);
            s_c[i] = c; s_g0[i] = g0; s_g1[i] = g1;
            if constexpr (NM) s_nm[i] = mg[2 * q + 1];
        }
        __syncthreads();
    }
    bool filt = false;
    if (x < W && y < H) {
        const size_t p = (size_t)y * a.width + (size_t)x;
        const uint32_t lp = (ly + 2u * S) * RW + lx + 2u * S;
        F4 cp, g0p, g1p = {0.0f, 0.0f, 0.0f, 0.0f}, np = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (S != 0) { cp = s_c[lp]; g0p = s_g0[lp]; }
        else { g0p = guides[2 * p]; cp = dn_record<FIRST, ALB, VAR>(in, half, mg, p, f2u(g0p.w) != kDnNoGeo); }
        const uint32_t matp = f2u(g0p.w);
        filt = matp != kDnNoGeo && dn_sampled<VAR>(cp);
        F4 o = cp;
        float sg = 0.0f, sgw = 0.0f;
        if constexpr (VAR) {
            if (filt) {
                // the prefilter: gv = the binomial mean of v over the 3 x 3 positions that count
#pragma unroll
                for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                    for (int dx = -1; dx <= 1; dx++) {
                        const float gg = dnv_g(dy, dx);
                        if constexpr (S != 0) {
                            const uint32_t lq = (uint32_t)((int)lp + dy * (int)RW + dx);
                            if (f2u(s_g0[lq].w) != matp) continue;
                            const float vq = s_c[lq].w;
                            if (vq < 0.0f) continue;
                            sg = sg + gg * vq; sgw = sgw + gg;
                        } else {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                            const size_t q = (size_t)qy * a.width + (size_t)qx;
                            if (f2u(guides[2 * q].w) != matp) continue;
                            const F4 cq = dn_record<FIRST, ALB, VAR>(in, half, mg, q, true);
                            if (!dn_sampled<VAR>(cq)) continue;
                            sg = sg + gg * cq.w; sgw = sgw + gg;
                        }
                    }
                }
            }
        }
        if constexpr (DBG) { dbg[2 * p] = filt ? cp.w : 0.0f; dbg[2 * p + 1] = filt ? sg / sgw : 0.0f; }
        else {
            if (filt) {
                float lum = 0.0f, inv = a.inv_sigma_color_s;
                if constexpr (VAR) { inv = dnv_inv(sg, sgw, sigma_var); lum = dnv_luma(cp.x, cp.y, cp.z); }
                if constexpr (S != 0) g1p = s_g1[lp]; else g1p = guides[2 * p + 1];
                if constexpr (!NM) np = g1p; else if constexpr (S != 0) np = s_nm[lp]; else np = mg[2 * p + 1];
                DnSum sum = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
                    for (int dx = -2; dx <= 2; dx++) {
                        const float hh = dn_h(dy) * dn_h(dx);
                        F4 g0q, cq, nq;
                        if constexpr (S != 0) {
                            const uint32_t lq = (uint32_t)((int)lp + (dy * (int)RW + dx) * (int)S);
                            g0q = s_g0[lq];
                            if (f2u(g0q.w) != matp) continue;
                            cq = s_c[lq];
                            if (!dn_sampled<VAR>(cq)) continue;
                            if constexpr (NM) nq = s_nm[lq]; else nq = s_g1[lq];
                        } else {
                            const int qx = x + s * dx, qy = y + s * dy;
                            if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                            const size_t q = (size_t)qy * a.width + (size_t)qx;
                            g0q = guides[2 * q];
                            if (f2u(g0q.w) != matp) continue;
                            cq = dn_record<FIRST, ALB, VAR>(in, half, mg, q, true);
                            if (!dn_sampled<VAR>(cq)) continue;
                            if constexpr (NM) nq = mg[2 * q + 1]; else nq = guides[2 * q + 1];
                        }
                        dn_tap<VAR>(sum, a, g0p, g1p, np, cp, lum, inv, g0q, nq, cq, hh);
                    }
                }
                o.x = sum.x / sum.w; o.y = sum.y / sum.w; o.z = sum.z / sum.w;
                if constexpr (VAR) o.w = sum.v / (sum.w * sum.w);
                if constexpr (ALB) { if (a.last) { const F4 A = mg[2 * p]; o.x = o.x * A.x; o.y = o.y * A.y; o.z = o.z * A.z; } }
            }
            if (a.last) o.w = 1.0f;
            out[p] = o;
        }
    }
    if constexpr (FIRST && !DBG) {
        const unsigned long long m = __ballot(filt);
        if (lane_id() == 0) s_cnt[threadIdx.x >> 6] = (uint32_t)__popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) partial[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
    }
}
// every form of both filters; mg is read only with a flag set (FL != 0), sigma_var only by VAR and half only by its first level: a caller passes 0 / null for what its form never reads
template <uint32_t S, bool FIRST, uint32_t FL, bool VAR>
__global__ __launch_bounds__(kBlock) void k_denoise_level(DenoiseLevel a, float sigma_var, const F4* __restrict__ in, const F4* __restrict__ half, const F4* __restrict__ guides, const F4* __restrict__ mg, F4* __restrict__ out, uint32_t* __restrict__ partial) {
    dn_level<S, FIRST, FL, VAR>(a, sigma_var, in, half, guides, mg, out, partial, nullptr);
}
// rtx_debug_denoise_variance: (v, gv) of level 0 per pixel
template <bool ALB>
__global__ __launch_bounds__(kBlock) void k_denoise_var_input(DenoiseLevel a, const F4* __restrict__ in, const F4* __restrict__ half, const F4* __restrict__ guides, const F4* __restrict__ mg, float* __restrict__ out2) {
    dn_level<0u, true, ALB ? kDnAlbedo : 0u, true, true>(a, 0.0f, in, half, guides, mg, nullptr, nullptr, out2);
}

// the filterable pixels of the image: the sum of the level-0 workgroups' counts (one workgroup, a plain store)
__global__ __launch_bounds__(kBlock) void k_denoise_count(const uint32_t* __restrict__ partial, uint32_t n, uint32_t* __restrict__ out) {
    __shared__ uint32_t s_sum[kBlock];
    uint32_t v = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) v += partial[i];
    s_sum[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t h = kBlock / 2; h > 0; h >>= 1) { if (threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h]; __syncthreads(); }
    if (threadIdx.x == 0) out[0] = s_sum[0];
}

}  // namespace rtx

// rtx_bvh_replay.cpp — host-side replay of the device traversal on the wide tree of a BuiltScene, and the commit-time any-hit probe built on it.  No HIP calls in this file.
#include "rtx_scene_host.hpp"
#include <cmath>

namespace rtx {

// ------------------------------------------------------------------------------------------------
// Host-side REPLAY of the device traversal (csrc/rtx_traverse.hpp: node8_hits / descend8 / traverse, one ray at a time, non-speculative order) on the
// wide tree of a BuiltScene, counting node steps and triangle tests.  Two users: tools/bvh_lab.cpp (builder work judged by work per ray, no GPU) and the
// commit-time probe below.  Scalar float code with the kernels' formulas; not bit-pinned to them (the counts, not the hits, are what it is for).
// ------------------------------------------------------------------------------------------------
namespace {
struct RGrp { uint32_t base, bits; };
struct RTri { uint32_t base, bits, valid; };
constexpr float kRPlaneEps = 2.384185791015625e-07f, kRSlabK = 1.00010002f;
inline void replay_node(const Node8GPU& N, const float o[3], const float idir[3], uint32_t oct, bool ordered, uint32_t oct_order, float tmin, float tbest, RGrp& G, RTri& T) {
    const uint32_t w = N.e_imask;
    const float s[3] = {u2f((w & 0xffu) << 23) * idir[0], u2f((w & 0xff00u) << 15) * idir[1], u2f((w & 0xff0000u) << 7) * idir[2]};
    const float a3[3] = {(N.px - o[0]) * idir[0], (N.py - o[1]) * idir[1], (N.pz - o[2]) * idir[2]};
    uint32_t hits = 0;
    for (int k = 0; k < 8; k++) {
        float lo = tmin, hi = tbest;
        for (int a = 0; a < 3; a++) {
            const uint32_t qlo = (N.q[2 * a + (k >> 2)] >> (8 * (k & 3))) & 0xffu, qhi = (N.q[2 * (3 + a) + (k >> 2)] >> (8 * (k & 3))) & 0xffu;
            const bool neg = (oct >> a) & 1u;
            const float an = fmaf(-fabsf(a3[a]), kRPlaneEps, a3[a]), af = fmaf(fabsf(a3[a]), kRPlaneEps, a3[a]);
            lo = fmaxf(lo, fmaf((float)(neg ? qhi : qlo), s[a], an)); hi = fminf(hi, fmaf((float)(neg ? qlo : qhi), s[a], af));
        }
        if (!(f2u(fmaf(hi, kRSlabK, -lo)) >> 31)) hits |= 1u << k;
    }
    const uint32_t imask = w >> 24;
    uint32_t m = hits & imask;
    if (ordered) { uint32_t pm = 0; for (int j = 0; j < 8; j++) if (m & (1u << (j ^ oct_order))) pm |= 1u << j; m = pm; }
    G.base = N.child_base; G.bits = m | (imask << 8);
    uint32_t x = hits & ~imask, sp = 0;
    for (int k = 0; k < 8; k++) if (x & (1u << k)) sp |= 0xfu << (4 * k);
    T.base = N.tri_base; T.valid = N.trivalid; T.bits = sp & N.trivalid;
}
inline bool replay_tri(const float o[3], const float d[3], const TriGPU& Tg, float tmin, float tmax, float& t) {
    const f3 v0 = mk3(Tg.v0.x, Tg.v0.y, Tg.v0.z), e1 = mk3(Tg.e1.x, Tg.e1.y, Tg.e1.z), e2 = mk3(Tg.e2.x, Tg.e2.y, Tg.e2.z), dd = mk3(d[0], d[1], d[2]);
    const f3 pv = cross(dd, e2);
    const float det = dot(e1, pv);
    if (!(fabsf(det) > Tg.e1.w)) return false;
    const float inv = 1.0f / det;
    const f3 sv = mk3(o[0], o[1], o[2]) - v0;
    const float u = dot(sv, pv) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    const f3 q = cross(sv, e1);
    const float v = dot(dd, q) * inv;
    if (!(v >= 0.0f && u + v <= 1.0f)) return false;
    t = dot(e2, q) * inv;
    return t > tmin && t < tmax;
}
}  // namespace

bool replay_tri_test(const float o[3], const float d[3], const TriGPU& Tg, float tmin, float tmax, float& t) { return replay_tri(o, d, Tg, tmin, tmax, t); }

ReplayHit replay_trace(const BuiltScene& B, const float o[3], const float d[3], float tmin, float tmax, bool any, uint32_t any_order, float t_known, std::vector<uint8_t>* seq) {
    float idir[3]; uint32_t oct = 0;
    for (int a = 0; a < 3; a++) { const float ds = fabsf(d[a]) < 1e-30f ? copysignf(1e-30f, d[a]) : d[a]; idir[a] = 1.0f / ds; if (idir[a] < 0.0f) oct |= 1u << a; }
    const bool ordered = !any || any_order != 0;
    const uint32_t oct_order = (any && any_order == 2) ? (oct ^ 7u) : oct;
    ReplayHit H{t_known > 0.0f ? t_known * 1.0000005f : tmax, 0xffffffffu, 0xffffffffu, 0u, 0u};
    if (B.nodes8.empty()) return H;
    RGrp stk[64]; int sp = 0;
    RGrp G{0u, (ordered ? (1u << oct_order) : 1u) | (1u << 8)};
    RTri T{0u, 0u, 0u};
    while (true) {
        if (G.bits & 0xffu) {
            const uint32_t k = (uint32_t)__builtin_ctz(G.bits), rest = G.bits & (G.bits - 1u);
            if ((rest & 0xffu) && sp < 64) stk[sp++] = RGrp{G.base, rest};
            const uint32_t slot = ordered ? (k ^ oct_order) : k;
            const uint32_t idx = G.base + (uint32_t)__builtin_popcount((G.bits >> 8) & ((1u << slot) - 1u));
            replay_node(B.nodes8[idx], o, idir, oct, ordered, oct_order, tmin, H.t, G, T);
            H.steps++;
            if (seq) seq->push_back((uint8_t)__builtin_popcount(T.bits));          // triangles this node step hands to the triangle steps
        }
        while (T.bits) {
            const uint32_t bit = (uint32_t)__builtin_ctz(T.bits);
            T.bits &= T.bits - 1u; H.tris++;
            const uint32_t slot = T.base + (uint32_t)__builtin_popcount(T.valid & ((1u << bit) - 1u));
            float t;
            if (replay_tri(o, d, B.tris8[slot], tmin, tmax, t)) {
                const uint32_t gid = f2u(B.tris8[slot].v0.w);
                if (any) { H.prim = gid; H.slot = slot; H.t = t; if (seq && !seq->empty()) seq->back() = (uint8_t)(seq->back() - __builtin_popcount(T.bits)); return H; }   // (the untested rest of the group is dropped)
                if (t < H.t || (t == H.t && gid < H.prim)) { H.t = t; H.prim = gid; H.slot = slot; }
            }
        }
        if (!(G.bits & 0xffu)) { if (sp == 0) break; G = stk[--sp]; }
    }
    return H;
}

// In which order should an any-hit ray visit the hit children of a node?  Any-hit is existence, so the order changes no result, only how soon an occluder is found:
// slot order (0), nearest octant first (1) or FARTHEST first (2: from the light's end — where a lamp's own housing, or the far faces of a closed emissive mesh, block
// the ray).  Which one wins is a property of the scene and its lights (Bistro-class street: far first -17 % node steps per occluded ray; the atrium under its sky
// quad: slot order), so it is probed once per commit: 2 048 NEE-like segments (a point on a random triangle to a CDF-sampled point on a light) replayed in the three
// orders; the cheapest by the traversal kernels' own cost model wins (node step 205 VALU at 47 of 64 lanes, triangle test 70 at 24), with 5 % hysteresis for order 0.
uint32_t probe_anyhit_order(const BuiltScene& B) {
    if (B.lights.empty() || B.tris8.empty() || B.nodes8.empty() || B.small_nrec) return 0u;
    auto h32 = [](uint32_t a, uint32_t b) { uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u; h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15; return h; };
    auto r01 = [&](uint32_t a, uint32_t b) { return (float)(h32(a, b) >> 8) * (1.0f / 16777216.0f); };
    double cost[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < 2048u; i++) {
        const TriGPU& Tg = B.tris8[h32(i, 1u) % (uint32_t)B.tris8.size()];
        float u = r01(i, 2u), v = r01(i, 3u); if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
        const f3 p = mk3(Tg.v0.x + u * Tg.e1.x + v * Tg.e2.x, Tg.v0.y + u * Tg.e1.y + v * Tg.e2.y, Tg.v0.z + u * Tg.e1.z + v * Tg.e2.z);
        f3 n = normalize(cross(mk3(Tg.e1.x, Tg.e1.y, Tg.e1.z), mk3(Tg.e2.x, Tg.e2.y, Tg.e2.z)));
        const float xi = r01(i, 4u);
        size_t li = 0; while (li + 1 < B.lights.size() && B.lights[li].cdf < xi) li++;
        const LightGPU& Lg = B.lights[li];
        float a = r01(i, 5u), b = r01(i, 6u); if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        const f3 lp = mk3(Lg.xv[0] + a * (Lg.yv[0] - Lg.xv[0]) + b * (Lg.zv[0] - Lg.xv[0]), Lg.xv[1] + a * (Lg.yv[1] - Lg.xv[1]) + b * (Lg.zv[1] - Lg.xv[1]), Lg.xv[2] + a * (Lg.yv[2] - Lg.xv[2]) + b * (Lg.zv[2] - Lg.xv[2]));
        f3 dir = lp - p;
        if (dot(n, dir) < 0.0f) n = mk3(-n.x, -n.y, -n.z);                      // surfaces are lit from either side
        const f3 org = mk3(p.x + kSBias * n.x, p.y + kSBias * n.y, p.z + kSBias * n.z);
        dir = lp - org;
        const float dist = length(dir);
        if (!(dist > 10.0f * kSBias)) continue;
        const float od[3] = {org.x, org.y, org.z}, dd[3] = {dir.x / dist, dir.y / dist, dir.z / dist};
        for (uint32_t ord = 0; ord < 3u; ord++) {
            const ReplayHit H = replay_trace(B, od, dd, 0.5f * kSBias, dist - 5.0f * kSBias, true, ord);
            cost[ord] += (double)H.steps * (205.0 * 64.0 / 47.0) + (double)H.tris * (70.0 * 64.0 / 24.0);
        }
    }
    uint32_t best = 0;
    for (uint32_t ord = 1; ord < 3u; ord++) if (cost[ord] < 0.95 * cost[0] && cost[ord] < cost[best]) best = ord;      // (an ordered step carries ~3 % more instructions)
    return best;
}

}  // namespace rtx

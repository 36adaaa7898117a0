// rtx_k_dbg.hpp — kernel-level debug probes of the parity tests
// One of the kernel headers of rtx_kernels.hip, the path tracer's single translation unit (see its header comment for the design and for why).
#pragma once
#include "rtx_shade.hpp"
#include "rtx_normalmap.hpp"
#include "rtx_specmap.hpp"

namespace rtx {

// ---------------------------------------------------------------------------------------------
// kernel-level debug entry points (parity tests): same device functions as the render loop
// ---------------------------------------------------------------------------------------------
template <bool CUT>      // CUT: the scene has a cut-out triangle — closest hit and any hit (modes 0 / 1) run the alpha test; the counted forms (modes 2 / 3: tree statistics, the any-hit order probe) never do
__global__ __launch_bounds__(kBlock) void k_dbg_trace(DevScene sc, const SmallRecPair* __restrict__ small, const F4* __restrict__ rays, uint32_t n, int any, F4* __restrict__ hits) {
    extern __shared__ F4 lds[];
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    const uint32_t stride = gridDim.x * kBlock;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
        const F4 ro = rays[2 * i], rd = rays[2 * i + 1];
        float t, u, v; uint32_t prim;
        if (any == 2) traverse<false, true>(sc, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w, rd.w, t, u, v, prim);
        else if (any == 3) traverse<true, true>(sc, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w, rd.w, t, u, v, prim);      // any-hit in the order sc.any_order, counted (u = node steps, v = triangle tests)
        else if (any) trace_ray<true, CUT>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w, rd.w, t, u, v, prim);
        else trace_ray<false, CUT>(sc, small, L, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), ro.w, rd.w, t, u, v, prim);
        hits[i] = {t, u, v, u2f(prim)};
    }
}
__global__ __launch_bounds__(kBlock) void k_dbg_surface(DevScene sc, const F4* __restrict__ rays, const F4* __restrict__ hits, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    F4 z = {0, 0, 0, 0};
    out[4 * i] = z; out[4 * i + 1] = z; out[4 * i + 2] = z; out[4 * i + 3] = z;
    if (f2u(h.w) == kMissPrim) { out[4 * i].w = u2f(kMissMat); return; }
    const F4 ro = rays[2 * i], rd = rays[2 * i + 1];
    const Surf s = surface(sc, mk3(ro.x, ro.y, ro.z), mk3(rd.x, rd.y, rd.z), h.x, h.y, h.z, f2u(h.w));
    out[4 * i] = {s.pos.x, s.pos.y, s.pos.z, u2f(s.mat)};
    out[4 * i + 1] = {s.normal.x, s.normal.y, s.normal.z, s.area};
    out[4 * i + 2] = {u2f(s.inst), s.flat.x, s.flat.y, s.flat.z};
}
__global__ __launch_bounds__(kBlock) void k_dbg_bsdf_eval(DevScene sc, uint32_t mat, uint32_t flags, const float* __restrict__ in9, uint32_t n, float* __restrict__ out8) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* q = in9 + (size_t)i * 9; float* o = out8 + (size_t)i * 8;
    f3 F; float P, pd, ps;
    f3 nrm = mk3(q[0], q[1], q[2]); const f3 wo = mk3(q[3], q[4], q[5]);
    const float eta_p = transmission_eta(sc.mats[mat], flags, wo, nrm);
    if (flags & 0x80000000u) {                       // the form k_shade runs: view terms computed once (MixView), mixture evaluated against them — must give the same bits
        const uint32_t fl = flags & 0x7FFFFFFFu;
        const MixView mv = mix_view(sc.mats[mat], fl, nrm, wo, eta_p);
        bsdf_mixture_v(sc.mats[mat], fl, mv, nrm, mk3(q[6], q[7], q[8]), wo, F, P, eta_p); pd = mv.pd; ps = mv.ps;
    } else bsdf_mixture(sc.mats[mat], flags, nrm, mk3(q[6], q[7], q[8]), wo, F, P, pd, ps, eta_p);
    o[0] = F.x; o[1] = F.y; o[2] = F.z; o[3] = P; o[4] = pd; o[5] = ps; o[6] = eta_p; o[7] = 0.0f;
}
__global__ __launch_bounds__(kBlock) void k_dbg_bsdf_sample(DevScene sc, uint32_t mat, uint32_t flags, const float* __restrict__ in8, uint32_t n, float* __restrict__ out8) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float* q = in8 + (size_t)i * 8; float* o = out8 + (size_t)i * 8;
    uint32_t s0 = f2u(q[6]), s1 = f2u(q[7]);
    f3 nrm = mk3(q[0], q[1], q[2]); const f3 wo = mk3(q[3], q[4], q[5]);
    const float eta_p = transmission_eta(sc.mats[mat], flags, wo, nrm);
    const uint32_t fl = flags & 0x7FFFFFFFu;
    const uint32_t st = (flags & 0x80000000u) ? select_strategy_v(sc.mats[mat], mix_view(sc.mats[mat], fl, nrm, wo, eta_p), fl, s0, s1, eta_p) : select_strategy(sc.mats[mat], wo, nrm, flags, s0, s1, eta_p);
    const f3 wi = sample_bsdf(sc.mats[mat], st, wo, nrm, s0, s1, eta_p);
    o[0] = wi.x; o[1] = wi.y; o[2] = wi.z; o[3] = u2f(st); o[4] = u2f(s0); o[5] = u2f(s1); o[6] = 0.0f; o[7] = 0.0f;
}
// the sampler and the per-hit albedo of the texture maps (rtx_texture.hpp), as k_shade<.., TEX> and debug layer 13 run them
__global__ __launch_bounds__(kBlock) void k_dbg_tex_sample(DevScene sc, uint32_t tex, const float* __restrict__ uv2, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const f3 c = tex_sample(sc, tex, uv2[2 * (size_t)i], uv2[2 * (size_t)i + 1]);
    out[i] = {c.x, c.y, c.z, 0.0f};
}
__global__ __launch_bounds__(kBlock) void k_dbg_albedo(DevScene sc, const F4* __restrict__ hits, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    const uint32_t prim = f2u(h.w);
    F4 r = {0.0f, 0.0f, 0.0f, u2f(0xFFFFFFFFu)};
    const uint32_t mat = prim != kMissPrim ? sc.shade[prim].mat : kMissMat;
    if (mat < sc.nmat) {
        int32_t tex;
        const f3 kd = tex_albedo(sc, sc.mats[mat], mat, prim, h.y, h.z, &tex);
        r = {kd.x, kd.y, kd.z, u2f((uint32_t)tex)};
    }
    out[i] = r;
}
// the alpha test of the cut-outs (rtx_cutout.hpp: cut_alpha, the function cut_accept compares with the cut-off) at n hit records -> (alpha, opacity texture id bits); (1, 0xFFFFFFFF)
// for a miss, for a triangle that is not a cut-out triangle and while no cut-out is active
__global__ __launch_bounds__(kBlock) void k_dbg_opacity(DevScene sc, const F4* __restrict__ hits, uint32_t n, float* __restrict__ out2) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    const uint32_t prim = f2u(h.w);
    float a = 1.0f; uint32_t id = 0xFFFFFFFFu;
    if (prim != kMissPrim && sc.tri_cut) {
        const int32_t tex = sc.tri_cut[prim];
        if (tex >= 0) { a = cut_alpha(sc, (uint32_t)tex, prim, h.y, h.z); id = (uint32_t)tex; }
    }
    out2[2 * (size_t)i] = a; out2[2 * (size_t)i + 1] = u2f(id);
}
// the shading normal of the normal maps (rtx_normalmap.hpp: nrm_perturb after surface(), as k_shade<.., NRM> runs them for a lane that shades) at n (ray, hit record) pairs ->
// (n', normal texture id bits); a miss gives (0, 0, 0, 0xFFFFFFFF); an emitter, a material without a map and every hit while no normal map is active give (surface()'s normal, 0xFFFFFFFF)
__global__ __launch_bounds__(kBlock) void k_dbg_shading_normal(DevScene sc, const F4* __restrict__ rays, const F4* __restrict__ hits, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    const uint32_t prim = f2u(h.w);
    F4 r = {0.0f, 0.0f, 0.0f, u2f(0xFFFFFFFFu)};
    if (prim != kMissPrim) {
        const F4 ro = rays[2 * i], rd = rays[2 * i + 1];
        const f3 d = mk3(rd.x, rd.y, rd.z);
        Surf sf = surface(sc, mk3(ro.x, ro.y, ro.z), d, h.x, h.y, h.z, prim);
        int32_t tex = -1;
        if (sc.tri_tan && sf.mat < sc.nmat && !(sc.mats[sf.mat].Ke_len > 0.0f)) sf.normal = nrm_perturb(sc, sf, prim, h.y, h.z, -d, &tex);
        r = {sf.normal.x, sf.normal.y, sf.normal.z, u2f((uint32_t)tex)};
    }
    out[i] = r;
}
// Ks', Pr', Pm' of the specular maps (rtx_specmap.hpp: spec_view, as k_shade<.., SPC> runs it for a lane that shades) at n hit records -> 8 words per record: Ks'.xyz, Pr',
// Pm', then the ks / pr / pm texture id bits; a miss gives five zeros and three 0xFFFFFFFF; an emitter and every hit while no specular map is active give the table's values
// and three 0xFFFFFFFF
__global__ __launch_bounds__(kBlock) void k_dbg_specular(DevScene sc, const F4* __restrict__ hits, uint32_t n, float* __restrict__ out8) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    const uint32_t prim = f2u(h.w);
    SpecView sv = {{0.0f, 0.0f, 0.0f}, 0.0f, 0.0f};
    int32_t tex[3] = {-1, -1, -1};
    if (prim != kMissPrim) {
        const uint32_t mat = sc.shade[prim].mat;
        if (mat < sc.nmat) {
            const MatGPU& m = sc.mats[mat];
            sv.Ks[0] = m.Ks[0]; sv.Ks[1] = m.Ks[1]; sv.Ks[2] = m.Ks[2]; sv.Pr = m.Pr; sv.Pm = m.Pm;
            if (sc.map_pr && !(m.Ke_len > 0.0f)) sv = spec_view(sc, m, mat, prim, h.y, h.z, tex);
        }
    }
    float* o = out8 + 8 * (size_t)i;
    o[0] = sv.Ks[0]; o[1] = sv.Ks[1]; o[2] = sv.Ks[2]; o[3] = sv.Pr; o[4] = sv.Pm;
    o[5] = u2f((uint32_t)tex[0]); o[6] = u2f((uint32_t)tex[1]); o[7] = u2f((uint32_t)tex[2]);
}
// the Ess the view terms of a hit on `material` take (mix_view: the energy table where spec_ess_table says so, else the material's LUT) at n (Pr', NdotV) pairs
__global__ __launch_bounds__(kBlock) void k_dbg_ess(DevScene sc, uint32_t material, const float* __restrict__ pr, const float* __restrict__ ndotv, uint32_t n, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const MatGPU& m = sc.mats[material];
    const float* tab = sc.map_pr ? spec_ess_table(sc, material) : nullptr;
    out[i] = tab ? ess_table(tab, sc.ess_rows, pr[i], ndotv[i]) : ess_lut(m, ndotv[i]);
}
// Ke' and q of the emission maps (rtx_emimap.hpp: emi_hit, as k_shade<.., EMI> runs it for a lane that hits an emitter) at n hit records -> 8 words per record: Ke'.xyz,
// q, the emission texture id bits, 0, 0, 0.  A non-emitter or a miss gives four zeros and 0xFFFFFFFF; while no emission map is active an emitter gives the table's Ke, the
// mean add_emissive forms of it and 0xFFFFFFFF
__global__ __launch_bounds__(kBlock) void k_dbg_emission(DevScene sc, const F4* __restrict__ hits, uint32_t n, float* __restrict__ out8) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const F4 h = hits[i];
    const uint32_t prim = f2u(h.w);
    EmiHit e; e.Ke = mk3(0.0f, 0.0f, 0.0f); e.q = 0.0f;
    int32_t tex = -1;
    if (prim != kMissPrim) {
        const uint32_t mat = sc.shade[prim].mat;
        if (mat < sc.nmat) {
            const MatGPU& m = sc.mats[mat];
            if (m.Ke_len > 0.0f) {
                if (sc.map_ke) e = emi_hit(sc, m, mat, prim, h.y, h.z, &tex);
                else { e.Ke = mk3(m.Ke[0], m.Ke[1], m.Ke[2]); e.q = (e.Ke.x + e.Ke.y + e.Ke.z) / 3.0f; }
            }
        }
    }
    float* o = out8 + 8 * (size_t)i;
    o[0] = e.Ke.x; o[1] = e.Ke.y; o[2] = e.Ke.z; o[3] = e.q; o[4] = u2f((uint32_t)tex); o[5] = 0.0f; o[6] = 0.0f; o[7] = 0.0f;
}
// the first half of a triangle-light NEE sample, statement for statement as nee_sample (rtx_shade.hpp) runs it — the CDF search on the selection draw, the two area draws and
// their fold, the sampled point — and the texel of the emission maps (emi_light_uv / emi_light_em) -> 12 words per seed: light index bits, the point, s, t, em * tl, pdf_l,
// the seed after the three draws.  A light without the map gives s = t = 0 and the record's em.  The launcher checks that the scene has a light list
__global__ __launch_bounds__(kBlock) void k_dbg_light_sample(DevScene sc, const uint32_t* __restrict__ seeds2, uint32_t n, float* __restrict__ out12) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t s0 = seeds2[2 * (size_t)i], s1 = seeds2[2 * (size_t)i + 1];
    const float rv = tea_next(s0, s1);
    int left = 0, right = (int)sc.nlights - 1, sel = 0;
    while (left <= right) {
        const int mid = left + (right - left) / 2;
        if (rv < sc.cdf[mid]) { sel = mid; right = mid - 1; } else left = mid + 1;
    }
    const LightGPU& lt = sc.lights[sel];
    const f3 xv = mk3(lt.xv[0], lt.xv[1], lt.xv[2]), yv = mk3(lt.yv[0], lt.yv[1], lt.yv[2]), zv = mk3(lt.zv[0], lt.zv[1], lt.zv[2]);
    float xi1 = tea_next(s0, s1), xi2 = tea_next(s0, s1);
    if (xi1 + xi2 > 1.0f) { xi1 = 1.0f - xi1; xi2 = 1.0f - xi2; }
    const float u = 1.0f - xi1 - xi2, v = xi1, w = xi2;
    const f3 sp = lincomb3(xv, u, yv, v, zv, w);
    float s = 0.0f, t = 0.0f;
    f3 em = mk3(lt.em[0], lt.em[1], lt.em[2]);
    if (sc.map_ke) { if (lt.emi_tex >= 0) emi_light_uv(sc, lt.prim, u, v, w, s, t); em = emi_light_em(sc, lt, u, v, w); }
    float* o = out12 + 12 * (size_t)i;
    o[0] = u2f((uint32_t)sel); o[1] = sp.x; o[2] = sp.y; o[3] = sp.z; o[4] = s; o[5] = t; o[6] = em.x; o[7] = em.y; o[8] = em.z; o[9] = lt.pdf_l; o[10] = u2f(s0); o[11] = u2f(s1);
}
// the environment's sampler and lookup (rtx_env.hpp), as k_shade<.., ENV> runs them (the marginal CDF from global memory: the same values as its LDS copy)
__global__ __launch_bounds__(kBlock) void k_dbg_env_sample(DevScene sc, const uint32_t* __restrict__ seeds2, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t s0 = seeds2[2 * (size_t)i], s1 = seeds2[2 * (size_t)i + 1];
    f3 Ln;
    const EnvEval E = env_sample(sc, sc.env_marg, s0, s1, Ln);
    out[3 * (size_t)i] = {Ln.x, Ln.y, Ln.z, E.pdf};
    out[3 * (size_t)i + 1] = {E.L.x, E.L.y, E.L.z, u2f(E.texel)};
    out[3 * (size_t)i + 2] = {u2f(s0), u2f(s1), 0.0f, 0.0f};
}
__global__ __launch_bounds__(kBlock) void k_dbg_env_eval(DevScene sc, const float* __restrict__ dirs3, uint32_t n, F4* __restrict__ out) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const EnvEval E = env_eval(sc, mk3(dirs3[3 * (size_t)i], dirs3[3 * (size_t)i + 1], dirs3[3 * (size_t)i + 2]));
    out[2 * (size_t)i] = {E.L.x, E.L.y, E.L.z, E.pdf};
    out[2 * (size_t)i + 1] = {u2f(E.texel), E.r3, 0.0f, 0.0f};
}
__global__ void k_dbg_tea(uint32_t s0, uint32_t s1, uint32_t n, float* __restrict__ out, uint32_t* __restrict__ seed_out) {
    if (threadIdx.x || blockIdx.x) return;
    for (uint32_t i = 0; i < n; i++) out[i] = tea_next(s0, s1);
    seed_out[0] = s0; seed_out[1] = s1;
}
// what the raygen kernels start a path with (camera_sample): the ray, resp. the seed state after its draws
template <bool LENS>
__global__ __launch_bounds__(kBlock) void k_dbg_primary(DevFrame f, const CameraGPU* __restrict__ cam, uint32_t sample_id, F4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= f.width * f.height) return;
    const uint32_t x = i % f.width, y = i / f.width;
    uint32_t s0, s1; f3 o, d;
    camera_sample<LENS>(*cam, f, x, y, sample_id, o, d, s0, s1);
    rays[2 * i] = {o.x, o.y, o.z, kTMinCam};
    rays[2 * i + 1] = {d.x, d.y, d.z, kTMax};
}
template <bool LENS>
__global__ __launch_bounds__(kBlock) void k_dbg_primary_seeds(DevFrame f, const CameraGPU* __restrict__ cam, uint32_t sample_id, uint32_t* __restrict__ seeds2) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= f.width * f.height) return;
    const uint32_t x = i % f.width, y = i / f.width;
    uint32_t s0, s1; f3 o, d;
    camera_sample<LENS>(*cam, f, x, y, sample_id, o, d, s0, s1);
    seeds2[2 * (size_t)i] = s0; seeds2[2 * (size_t)i + 1] = s1;
}
// rtx_focus_distance_at: the first hit of pixel (x, y)'s pixel-corner pinhole ray, as the debug layers trace it (for_each_first_hit, rtx_k_film.hpp), as a depth along the view
// axis: t * cz, 0 on a miss.  One workgroup (it stages the scene's LDS); every lane traces the same ray, lane 0 stores
template <bool CUT>
__global__ __launch_bounds__(kBlock) void k_focus_distance(DevScene sc, const SmallRecPair* __restrict__ small, uint32_t width, uint32_t height, const CameraGPU* __restrict__ cam, uint32_t x, uint32_t y, float* __restrict__ out) {
    extern __shared__ F4 lds[];
    const TraceLds L = stage_lds(sc, lds);
    __syncthreads();
    f3 o, d; primary_ray(*cam, width, height, x, y, 0.0f, 0.0f, o, d);
    float t, u, v; uint32_t prim;
    trace_ray<false, CUT>(sc, small, L, o, d, kTMinCam, kTMax, t, u, v, prim);
    if (threadIdx.x == 0) out[0] = prim != kMissPrim ? t * view_axis_cos(*cam, d) : 0.0f;
}

}  // namespace rtx

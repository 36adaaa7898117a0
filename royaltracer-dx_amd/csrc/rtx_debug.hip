// rtx_debug.hip — the rtx_debug_* entry points of include/rtx.h: single kernels on caller-supplied rays and materials, the tree as the device and the host hold it,
// build times, work counters.  Tooling and tests; no frame goes through here (rtx_ctx.hpp).
#include "rtx_ctx.hpp"

// The body the per-hit probes of the map slots share: n hit records as rtx_debug_trace_closest writes them (and, for a probe that takes them, the n rays behind them) go to the
// device, launch(rays, hits, out) runs the probe's kernel, out_item bytes per record come back.  Checked in this order: committed, n == 0, null arrays ("<name>: null array"),
// triangle ids ("<name>: triangle id out of range": an id the scene does not have would index past the per-triangle tables)
template <class Launch>
static int hit_probe(rtx_ctx* c, const char* name, bool takes_rays, const float* rays8, const float* hits4, uint32_t n, void* out, size_t out_item, Launch launch) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    if ((takes_rays && !rays8) || !hits4 || !out) { c->err = std::string(name) + ": null array"; return RTX_ERR_INVALID; }
    for (uint32_t i = 0; i < n; i++) {
        uint32_t prim; memcpy(&prim, &hits4[(size_t)i * 4 + 3], 4);
        if (prim != kMissPrim && prim >= c->stats.triangles) { c->err = std::string(name) + ": triangle id out of range"; return RTX_ERR_INVALID; }
    }
    DevBuf d_rays, d_hits, d_out;
    if (takes_rays) { HIPCHK(c, d_rays.ensure((size_t)n * 32)); TO_DEVICE(c, d_rays.p, rays8, (size_t)n * 32); }
    HIPCHK(c, d_hits.ensure((size_t)n * 16)); HIPCHK(c, d_out.ensure((size_t)n * out_item));
    TO_DEVICE(c, d_hits.p, hits4, (size_t)n * 16);
    launch((const F4*)d_rays.p, (const F4*)d_hits.p, d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out, d_out.p, (size_t)n * out_item);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

extern "C" {

int rtx_debug_primary_rays(rtx_ctx* c, const rtx_params* p, uint32_t sample_id, float* rays8) {
    BIND(c);
    if (!c->camera_set) { c->err = "camera not set"; return RTX_ERR_STATE; }
    DevFrame f; int r = make_frame(c, p, f); if (r) return r;
    DevBuf d_rays; const size_t n = (size_t)p->width * p->height;
    HIPCHK(c, d_rays.ensure(n * 32));
    launch_dbg_primary(c->stream, f, (const CameraGPU*)c->d_cam.p, sample_id, (F4*)d_rays.p);
    TO_HOST(c, rays8, d_rays.p, n * 32);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
int rtx_debug_primary_seeds(rtx_ctx* c, const rtx_params* p, uint32_t sample_id, uint32_t* seeds2) {
    BIND(c);
    if (!c->camera_set) { c->err = "camera not set"; return RTX_ERR_STATE; }
    if (!seeds2) { c->err = "primary_seeds: null array"; return RTX_ERR_INVALID; }
    DevFrame f; int r = make_frame(c, p, f); if (r) return r;
    DevBuf d_seeds; const size_t n = (size_t)p->width * p->height;
    HIPCHK(c, d_seeds.ensure(n * 8));
    launch_dbg_primary_seeds(c->stream, f, (const CameraGPU*)c->d_cam.p, sample_id, (uint32_t*)d_seeds.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, seeds2, d_seeds.p, n * 8);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
static int dbg_trace(rtx_ctx* c, const float* rays8, uint32_t n, int any, float* hits4, uint8_t* occ) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    DevBuf d_rays, d_hits;
    HIPCHK(c, d_rays.ensure((size_t)n * 32)); HIPCHK(c, d_hits.ensure((size_t)n * 16));
    TO_DEVICE(c, d_rays.p, rays8, (size_t)n * 32);
    launch_dbg_trace(c->stream, c->dsc, (const F4*)d_rays.p, n, any, (F4*)d_hits.p);
    HIPCHK(c, hipGetLastError());
    std::vector<float> h((size_t)n * 4);
    TO_HOST(c, h.data(), d_hits.p, (size_t)n * 16);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hits4) memcpy(hits4, h.data(), (size_t)n * 16);
    if (occ) for (uint32_t i = 0; i < n; i++) { uint32_t prim; memcpy(&prim, &h[(size_t)i * 4 + 3], 4); occ[i] = prim != kMissPrim; }
    return RTX_OK;
}
int rtx_debug_trace_closest(rtx_ctx* c, const float* rays8, uint32_t n, float* hits4) { return dbg_trace(c, rays8, n, 0, hits4, nullptr); }
int rtx_debug_trace_any(rtx_ctx* c, const float* rays8, uint32_t n, uint8_t* occluded) { return dbg_trace(c, rays8, n, 1, nullptr, occluded); }
int rtx_debug_validate_bvh(rtx_ctx* c) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    std::vector<Node8GPU> nodes(c->dsc.nnodes); std::vector<TriGPU> tris(c->dsc.ntris);
    if (!nodes.empty()) TO_HOST(c, nodes.data(), c->scene.d_nodes.p, nodes.size() * sizeof(Node8GPU));
    if (!tris.empty()) TO_HOST(c, tris.data(), c->scene.d_tris.p, tris.size() * sizeof(TriGPU));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // the triangle the kernels intersect: (v0, v0 + e1, v0 + e2), filed under its global id (v0.w): a spatial split references a triangle from several leaf entries
    uint32_t ng = 0;
    for (const TriGPU& T : tris) ng = std::max(ng, f2u(T.v0.w) + 1u);
    std::vector<float> w((size_t)ng * 9, 0.0f); std::vector<uint32_t> ident(tris.size()), gid(tris.size());
    for (size_t i = 0; i < tris.size(); i++) {
        const TriGPU& T = tris[i]; ident[i] = (uint32_t)i; gid[i] = f2u(T.v0.w); float* o = &w[(size_t)gid[i] * 9];
        o[0] = T.v0.x; o[1] = T.v0.y; o[2] = T.v0.z; o[3] = T.v0.x + T.e1.x; o[4] = T.v0.y + T.e1.y; o[5] = T.v0.z + T.e1.z; o[6] = T.v0.x + T.e2.x; o[7] = T.v0.y + T.e2.y; o[8] = T.v0.z + T.e2.z;
    }
    // hidden instances (rtx_set_instance_visible): the never-hit marker e1.w = +inf must sit on exactly the triangles of the instances committed as hidden (code 27), and the
    // hidden triangles may widen no box (validate_bvh8).  The leaf padding is the refit kernels': 2e-6 x the coordinate scale the device holds
    const BuiltScene& B = c->scene.built;
    std::vector<uint8_t> hidden(tris.size(), 0); bool any = false;
    for (size_t i = 0; i < tris.size(); i++) {
        hidden[i] = tris[i].e1.w == INFINITY ? 1 : 0; any = any || hidden[i];
        size_t ii = (size_t)(std::upper_bound(c->host.insts.begin(), c->host.insts.end(), gid[i], [](uint32_t v, const InstHost& in) { return v < in.tri_base; }) - c->host.insts.begin());      // one past the last instance starting at or before the triangle
        const bool want = ii > 0 && ii - 1 < B.inst_hidden.size() && B.inst_hidden[ii - 1] != 0u;
        if (want != (hidden[i] != 0)) return 27;
    }
    if (!any) return validate_bvh8(w, nodes, gid, ident, nullptr);
    float scale = 1.0f;
    if (c->scene.node_aabb_valid && c->scene.d_scale.p) { TO_HOST(c, &scale, c->scene.d_scale.p, 4); }
    return validate_bvh8(w, nodes, gid, ident, nullptr, &hidden, 2e-6 * (double)scale);
}
int rtx_debug_tree_hash(rtx_ctx* c, uint64_t out2[2]) {
    BIND(c);
    if (!c->committed || !out2) { if (c) c->err = "scene not committed"; return RTX_ERR_STATE; }
    std::vector<uint8_t> nodes((size_t)c->scene.n_nodes8 * sizeof(Node8GPU)), tris((size_t)c->scene.n_tris8 * sizeof(TriGPU));
    if (!nodes.empty()) TO_HOST(c, nodes.data(), c->scene.d_nodes.p, nodes.size());
    if (!tris.empty()) TO_HOST(c, tris.data(), c->scene.d_tris.p, tris.size());
    HIPCHK(c, hipStreamSynchronize(c->stream));
    auto fnv = [](const std::vector<uint8_t>& v) { uint64_t h = 1469598103934665603ull; for (uint8_t b : v) { h ^= b; h *= 1099511628211ull; } return h; };
    out2[0] = fnv(nodes); out2[1] = fnv(tris);
    return RTX_OK;
}
int rtx_debug_tree_cost(rtx_ctx* c, double out2[2]) {
    BIND(c);
    if (!out2) { c->err = "tree_cost: null array"; return RTX_ERR_INVALID; }
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    return tree_costs(c, out2);
}
int rtx_debug_read_tree(rtx_ctx* c, int which, void* nodes, uint64_t nodes_bytes, void* tris, uint64_t tris_bytes) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    const size_t nb = (size_t)c->scene.n_nodes8 * sizeof(Node8GPU), tb = (size_t)c->scene.n_tris8 * sizeof(TriGPU);
    if ((nodes && nodes_bytes != nb) || (tris && tris_bytes != tb)) { c->err = "read_tree: buffers must hold rtx_stats.bvh_nodes * 80 and bvh_refs * 48 bytes"; return RTX_ERR_INVALID; }
    if (which == 0) {
        if (nodes) TO_HOST(c, nodes, c->scene.d_nodes.p, nb);
        if (tris) TO_HOST(c, tris, c->scene.d_tris.p, tb);
        return RTX_OK;
    }
    const BuiltScene& B = c->scene.built;
    if (B.nodes8.size() != c->scene.n_nodes8 || B.tris8.size() != c->scene.n_tris8) { c->err = "read_tree: the host holds no mirror of this tree (built on the device, or loaded without one)"; return RTX_ERR_STATE; }
    if (nodes) memcpy(nodes, B.nodes8.data(), nb);
    if (tris) memcpy(tris, B.tris8.data(), tb);
    return RTX_OK;
}
int rtx_debug_read_host_build(rtx_ctx* c, void* nodes2, uint64_t* nodes2_bytes, void* leaf_order, uint64_t* leaf_order_bytes) {
    if (!c || !nodes2_bytes || !leaf_order_bytes) return RTX_ERR_INVALID;
    const BuiltScene& B = c->scene.built;
    const uint64_t nb = (uint64_t)B.nodes.size() * sizeof(NodeGPU), lb = (uint64_t)B.leaf_order.size() * 4u;
    if (nodes2 && *nodes2_bytes >= nb) memcpy(nodes2, B.nodes.data(), (size_t)nb);
    if (leaf_order && *leaf_order_bytes >= lb) memcpy(leaf_order, B.leaf_order.data(), (size_t)lb);
    *nodes2_bytes = nb; *leaf_order_bytes = lb;
    return RTX_OK;
}
int rtx_debug_host_checksums(rtx_ctx* c, uint64_t out8[8]) {
    if (!c || !out8) return RTX_ERR_INVALID;
    auto fnv = [](uint64_t h, const void* d, size_t n) { const uint8_t* q = (const uint8_t*)d; for (size_t i = 0; i < n; i++) { h ^= q[i]; h *= 1099511628211ull; } return h; };
    for (int k = 0; k < 8; k++) out8[k] = 1469598103934665603ull;
    const SceneHost& H = c->host; const BuiltScene& B = c->scene.built;
    for (const MeshHost& m : H.meshes) { out8[0] = fnv(out8[0], m.idx.data(), m.idx.size() * 4); out8[1] = fnv(out8[1], m.verts.data(), m.verts.size() * 4); }
    out8[2] = fnv(fnv(out8[2], H.matids.data(), H.matids.size() * 4), H.mats128.data(), H.mats128.size() * 4);
    out8[3] = fnv(out8[3], H.insts.data(), H.insts.size() * sizeof(InstHost));
    out8[4] = fnv(out8[4], B.leaf_order.data(), B.leaf_order.size() * 4);
    out8[5] = fnv(out8[5], B.nodes.data(), B.nodes.size() * sizeof(NodeGPU));
    out8[6] = fnv(fnv(out8[6], B.nodes8.data(), B.nodes8.size() * sizeof(Node8GPU)), B.tris8.data(), B.tris8.size() * sizeof(TriGPU));
    out8[7] = fnv(fnv(fnv(out8[7], B.shade.data(), B.shade.size() * sizeof(TriShade)), B.objtris.data(), B.objtris.size() * sizeof(F4)), B.tri_slots8.data(), B.tri_slots8.size() * 4);
    return RTX_OK;
}
int rtx_debug_build_info(rtx_ctx* c, double ms5[5], uint32_t counts4[4]) {
    if (!c || !ms5 || !counts4) return RTX_ERR_INVALID;
    const GpuBuildResult& G = c->scene.build_info;
    const bool g = c->scene.dev_built;
    ms5[0] = g ? G.ms_prims : 0; ms5[1] = g ? G.ms_sort : 0; ms5[2] = g ? G.ms_ploc : 0; ms5[3] = g ? G.ms_top_host : 0; ms5[4] = g ? G.ms_layout : 0;
    counts4[0] = c->scene.n_nodes8; counts4[1] = c->scene.n_tris8; counts4[2] = g ? G.ploc_iterations : 0; counts4[3] = g ? G.clusters_top : 0;
    return RTX_OK;
}
// work counters of the persistent traversal kernels since they were last read (RTX_OPT_TRACE_COUNTERS 1): out4 = node steps and triangle tests of closest-hit rays, node steps and
// triangle tests of any-hit rays; reading resets them.  Rays per class: rtx_stats (rays_primary + rays_extension, rays_shadow)
int rtx_debug_trace_counters(rtx_ctx* c, uint64_t out4[4]) {
    BIND(c);
    if (!c->opt.trace_counters || !c->d_trace_cnt.p) { c->err = "trace counters are off (RTX_OPT_TRACE_COUNTERS)"; return RTX_ERR_STATE; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->pt.aux) HIPCHK(c, hipStreamSynchronize(c->pt.aux));
    unsigned long long h[4];
    TO_HOST(c, h, c->d_trace_cnt.p, 32);
    HIPCHK(c, hipMemset(c->d_trace_cnt.p, 0, 32));
    for (int i = 0; i < 4; i++) out4[i] = h[i];
    return RTX_OK;
}
int rtx_debug_trace_stats(rtx_ctx* c, const float* rays8, uint32_t n, float* stats4) { return dbg_trace(c, rays8, n, 2, stats4, nullptr); }

int rtx_debug_surface(rtx_ctx* c, const float* rays8, const float* hits4, uint32_t n, float* out16) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    DevBuf d_rays, d_hits, d_out;
    HIPCHK(c, d_rays.ensure((size_t)n * 32)); HIPCHK(c, d_hits.ensure((size_t)n * 16)); HIPCHK(c, d_out.ensure((size_t)n * 64));
    TO_DEVICE(c, d_rays.p, rays8, (size_t)n * 32);
    TO_DEVICE(c, d_hits.p, hits4, (size_t)n * 16);
    launch_dbg_surface(c->stream, c->dsc, (const F4*)d_rays.p, (const F4*)d_hits.p, n, (F4*)d_out.p);
    HIPCHK(c, hipGetLastError());
    std::vector<float> h((size_t)n * 16);
    TO_HOST(c, h.data(), d_out.p, (size_t)n * 64);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    // device layout: pos3,mat | normal3,area | inst,flat3 | 0  ->  API layout: pos3,mat,normal3,area,inst,flat3,pad4
    memcpy(out16, h.data(), (size_t)n * 64);
    return RTX_OK;
}
// the shading normal under the normal maps (rtx_normalmap.hpp), by the device functions k_shade<.., NRM> runs for a lane that shades
int rtx_debug_shading_normal(rtx_ctx* c, const float* rays8, const float* hits4, uint32_t n, float* out4) {
    return hit_probe(c, "shading_normal", true, rays8, hits4, n, out4, 16, [&](const F4* rays, const F4* hits, void* out) { launch_dbg_shading_normal(c->stream, c->dsc, rays, hits, n, (F4*)out); });
}
// the per-hit diffuse colour under the diffuse maps (rtx_texture.hpp).  rays8 is taken for symmetry with rtx_debug_surface; the albedo depends on the hit record alone
// (triangle id and barycentrics)
int rtx_debug_albedo(rtx_ctx* c, const float* rays8, const float* hits4, uint32_t n, float* out4) {
    (void)rays8;
    return hit_probe(c, "albedo", false, nullptr, hits4, n, out4, 16, [&](const F4*, const F4* hits, void* out) { launch_dbg_albedo(c->stream, c->dsc, hits, n, (F4*)out); });
}
// (alpha as the traversal computes it, opacity texture id as uint bits): cut_alpha of rtx_cutout.hpp, the function cut_accept compares
int rtx_debug_opacity(rtx_ctx* c, const float* hits4, uint32_t n, float* out2) {
    return hit_probe(c, "opacity", false, nullptr, hits4, n, out2, 8, [&](const F4*, const F4* hits, void* out) { launch_dbg_opacity(c->stream, c->dsc, hits, n, (float*)out); });
}
int rtx_debug_tri_tangents(rtx_ctx* c, uint32_t first, uint32_t count, float* out6) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!c->dsc.tri_tan) { c->err = "tri_tangents: no normal map is active"; return RTX_ERR_STATE; }
    if ((uint64_t)first + count > c->stats.triangles) { c->err = "tri_tangents: triangle range out of bounds"; return RTX_ERR_INVALID; }
    if (!count) return RTX_OK;
    if (!out6) { c->err = "tri_tangents: null array"; return RTX_ERR_INVALID; }
    TO_HOST(c, out6, (const char*)c->scene.d_tri_tan.p + (size_t)first * 24, (size_t)count * 24);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
// Ks', Pr', Pm' under the specular maps (rtx_specmap.hpp), by the device function k_shade<.., SPC> runs for a lane that shades
int rtx_debug_specular(rtx_ctx* c, const float* hits4, uint32_t n, float* out8) {
    return hit_probe(c, "specular", false, nullptr, hits4, n, out8, 32, [&](const F4*, const F4* hits, void* out) { launch_dbg_specular(c->stream, c->dsc, hits, n, (float*)out); });
}
// the Ess the view terms take for `material` at n (Pr', NdotV) pairs: the energy table where the material has a roughness map and a table is set, else its own LUT
int rtx_debug_ess(rtx_ctx* c, uint32_t material, const float* pr, const float* ndotv, uint32_t n, float* out) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (material >= c->dsc.nmat) { c->err = "ess: unknown material"; return RTX_ERR_INVALID; }
    if (!n) return RTX_OK;
    if (!pr || !ndotv || !out) { c->err = "ess: null array"; return RTX_ERR_INVALID; }
    DevBuf d_pr, d_nv, d_out;
    HIPCHK(c, d_pr.ensure((size_t)n * 4)); HIPCHK(c, d_nv.ensure((size_t)n * 4)); HIPCHK(c, d_out.ensure((size_t)n * 4));
    TO_DEVICE(c, d_pr.p, pr, (size_t)n * 4);
    TO_DEVICE(c, d_nv.p, ndotv, (size_t)n * 4);
    launch_dbg_ess(c->stream, c->dsc, material, (const float*)d_pr.p, (const float*)d_nv.p, n, (float*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out, d_out.p, (size_t)n * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
// Ke' and q under the emission maps (rtx_emimap.hpp), by the device function k_shade<.., EMI> runs for a lane that hits an emitter
int rtx_debug_emission(rtx_ctx* c, const float* hits4, uint32_t n, float* out8) {
    return hit_probe(c, "emission", false, nullptr, hits4, n, out8, 32, [&](const F4*, const F4* hits, void* out) { launch_dbg_emission(c->stream, c->dsc, hits, n, (float*)out); });
}
// the first half of a triangle-light NEE sample with the texel of the emission maps, by the device functions nee_sample runs
int rtx_debug_light_sample(rtx_ctx* c, const uint32_t* seeds2, uint32_t n, float* out12) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (!c->dsc.nlights) { c->err = "light_sample: the scene has no light list (no emitter, or every emission map black)"; return RTX_ERR_STATE; }
    if (!n) return RTX_OK;
    if (!seeds2 || !out12) { c->err = "light_sample: null array"; return RTX_ERR_INVALID; }
    DevBuf d_in, d_out;
    HIPCHK(c, d_in.ensure((size_t)n * 8)); HIPCHK(c, d_out.ensure((size_t)n * 48));
    TO_DEVICE(c, d_in.p, seeds2, (size_t)n * 8);
    launch_dbg_light_sample(c->stream, c->dsc, (const uint32_t*)d_in.p, n, (float*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out12, d_out.p, (size_t)n * 48);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
static int dbg_bsdf(rtx_ctx* c, bool sample, uint32_t mat, uint32_t flags, const float* in, uint32_t stride_in, uint32_t n, float* out8) {
    BIND(c);
    if (!c->committed) { c->err = "scene not committed"; return RTX_ERR_STATE; }
    if (mat >= c->dsc.nmat) { c->err = "material id out of range"; return RTX_ERR_INVALID; }
    if (!n) return RTX_OK;
    DevBuf d_in, d_out;
    HIPCHK(c, d_in.ensure((size_t)n * stride_in * 4)); HIPCHK(c, d_out.ensure((size_t)n * 32));
    TO_DEVICE(c, d_in.p, in, (size_t)n * stride_in * 4);
    if (sample) launch_dbg_bsdf_sample(c->stream, c->dsc, mat, flags, (const float*)d_in.p, n, (float*)d_out.p);
    else launch_dbg_bsdf_eval(c->stream, c->dsc, mat, flags, (const float*)d_in.p, n, (float*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out8, d_out.p, (size_t)n * 32);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
int rtx_debug_bsdf_eval(rtx_ctx* c, uint32_t mat, uint32_t flags, const float* in9, uint32_t n, float* out8) { return dbg_bsdf(c, false, mat, flags, in9, 9, n, out8); }
int rtx_debug_bsdf_sample(rtx_ctx* c, uint32_t mat, uint32_t flags, const float* in8, uint32_t n, float* out8) { return dbg_bsdf(c, true, mat, flags, in8, 8, n, out8); }

int rtx_debug_tea(rtx_ctx* c, uint32_t seed[2], uint32_t n, float* out) {
    BIND(c);
    if (!seed || !out) return RTX_ERR_INVALID;
    DevBuf d_out, d_seed;
    HIPCHK(c, d_out.ensure((size_t)std::max<uint32_t>(n, 1) * 4)); HIPCHK(c, d_seed.ensure(8));
    launch_dbg_tea(c->stream, seed[0], seed[1], n, (float*)d_out.p, (uint32_t*)d_seed.p);
    HIPCHK(c, hipGetLastError());
    if (n) TO_HOST(c, out, d_out.p, (size_t)n * 4);
    TO_HOST(c, seed, d_seed.p, 8);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"

// rtx_commit.hip — rtx_commit_scene: the scene's device arrays from a host build (or a host refit), a GPU build (RTX_OPT_GPU_BUILD) or a GPU refit; the scene cache;
// finalise_scene, which derives what the kernels read (DevScene) and the LDS budget.  Part of the C-ABI of include/rtx.h (rtx_ctx.hpp).
#include "rtx_ctx.hpp"

void pick_lds_closest(rtx_ctx* c) {
    DevScene& s = c->dsc;
    // ... and the CLOSEST-HIT launches of the path tracer take the other side of that trade (round 4, after the queue order was tightened): with the first three levels of the
    // wide tree in LDS (73 nodes) and six workgroups per CU they run C3 20.5 -> 19.6 ms and C5 17.3 -> 17.0 ms per frame against eight / seven workgroups with 24 / 31 nodes,
    // while the shadow launches lose (11.1 -> 12.2 ms on C3): a closest-hit ray crosses the top of the tree at every step of its front-to-back walk, an any-hit ray leaves at
    // its first occluder.  So the count is per kind of launch (DevScene goes by value).  Fewer than six workgroups lose again (128 nodes on C3: 20.4 ms; 80 on C5: 17.6).
    // LDS granule: the measurements fit 1 KB (80 nodes on C5 "fit" six workgroups at 512 B and ran like five).
    c->scene.lds_nodes_closest = 0;
    // In a frame the shadow launch of bounce b runs BESIDE the closest-hit launch of bounce b + 1 (RTX_OPT_OVERLAP_SHADOW), and six closest-hit workgroups of 25 KB leave it
    // no LDS on that CU: the street scene (30 MB of nodes, closest-hit kernel co-limited by memory, so the overlap is worth more there) LOSES 0.4 ms per frame with 73
    // nodes although the kernel alone gains 0.3; the atrium (2.2 MB of nodes) keeps 0.15-0.2 of the kernel's 0.9 ms (one context, option switched between rounds).  Auto therefore applies to trees that fit L2 (<= 16 MB,
    // the same line the wide node copy draws); RTX_OPT_LDS_NODES_CLOSEST sets it by hand.
    const bool small_tree = (size_t)s.nnodes * sizeof(Node8GPU) <= ((size_t)16 << 20);
    if (!s.nsmall && s.nnodes > s.lds_nodes && c->opt.lds_nodes_opt < 0 && (c->opt.lds_closest_opt >= 0 || small_tree)) {
        auto fit1k = [&](uint32_t nodes) { DevScene t = s; t.lds_nodes = nodes; return (160u * 1024u) / (uint32_t)((trace_lds_bytes(t) + 64 + 1023) & ~(size_t)1023); };
        uint32_t n = c->opt.lds_closest_opt >= 0 ? std::min<uint32_t>((uint32_t)c->opt.lds_closest_opt, s.nnodes) : std::min<uint32_t>(73u, s.nnodes);
        if (c->opt.lds_closest_opt < 0) while (n > s.lds_nodes && fit1k(n) < 6u) n--;
        DevScene t = s; t.lds_nodes = n;
        if (n > s.lds_nodes && trace_lds_bytes(t) <= 64 * 1024) c->scene.lds_nodes_closest = n;
    }
}

extern "C" {

static int upload_lights(rtx_ctx* c) {         // the light records and their CDF as a dense float array (DevScene::cdf)
    const BuiltScene& B = c->scene.built;
    std::vector<float>& cdf = c->scene.h_cdf;           // (a member: the source of an asynchronous copy must outlive the call)
    cdf.resize(B.lights.size());
    for (size_t i = 0; i < cdf.size(); i++) cdf[i] = B.lights[i].cdf;
    int r = upload(c, c->scene.d_lights, B.lights);
    if (r) return r;
    if (B.emi_q.empty()) c->scene.d_emi_q.release();       // (emission maps: q per global triangle id travels with the list it was built with)
    else if ((r = upload(c, c->scene.d_emi_q, B.emi_q))) return r;
    if (B.lights_plain.empty()) { c->scene.d_lights_plain.release(); c->scene.d_cdf_plain.release(); }      // (... and so does the unmapped scene's list)
    else {
        std::vector<float>& pc = c->scene.h_cdf_plain;
        pc.resize(B.lights_plain.size());
        for (size_t i = 0; i < pc.size(); i++) pc[i] = B.lights_plain[i].cdf;
        if ((r = upload(c, c->scene.d_lights_plain, B.lights_plain)) || (r = upload(c, c->scene.d_cdf_plain, pc))) return r;
    }
    return upload(c, c->scene.d_cdf, cdf);
}
static int upload_built(rtx_ctx* c) {          // every device array of a freshly built (or freshly loaded) scene
    BuiltScene& B = c->scene.built;
    int r;
    if ((r = upload(c, c->scene.d_nodes, B.nodes8))) return r;
    if ((r = upload(c, c->scene.d_tris, B.tris8))) return r;
    c->scene.n_nodes8 = (uint32_t)B.nodes8.size(); c->scene.n_tris8 = (uint32_t)B.tris8.size(); c->scene.dev_built = false;
    if (!B.nodes8.empty()) c->scene.root8 = B.nodes8[0]; else memset(&c->scene.root8, 0, sizeof(c->scene.root8));
    if ((r = upload(c, c->scene.d_shade, B.shade))) return r;
    if ((r = upload(c, c->scene.d_small, B.small_recs))) return r;
    if ((r = upload(c, c->scene.d_small_tris, B.small_tris))) return r;
    if ((r = upload(c, c->scene.d_small_poly, B.small_poly))) return r;
    if ((r = upload(c, c->scene.d_small_slabs, B.small_slabs))) return r;
    if ((r = upload(c, c->scene.d_mats, B.mats))) return r;
    if ((r = upload(c, c->scene.d_insts, B.insts))) return r;
    return upload_lights(c);
}
static int finalise_scene(rtx_ctx* c);

// byte -> float of a texel channel (include/rtx.h, rtx_set_texture): [0, 256) linear, [256, 512) sRGB decoded in double and rounded once
// ... and behind them [512, 768) the decode table of the normal maps: Nt[b] = max(((float)b - 128.0f) / 127.0f, -1.0f); byte 128 is exactly 0, byte 255 exactly 1
static void fill_tex_lut(std::vector<float>& lut) {
    lut.resize(768);
    for (int b = 0; b < 256; b++) {
        lut[512 + b] = std::max(((float)b - 128.0f) / 127.0f, -1.0f);
        lut[b] = (float)b / 255.0f;
        const double cs = b / 255.0;
        lut[256 + b] = (float)(cs <= 0.04045 ? cs / 12.92 : pow((cs + 0.055) / 1.055, 2.4));
    }
}
// The device's texture tables follow the host's (SceneHost::textures / maps / MeshHost::uvs): tables only, no kernel runs.  renumbered: this commit numbered the global
// triangle ids anew (a build); deformed: a mesh got new vertices (the tangent records are derived from them).  What the kernels see of it is set by finalise_scene.
static int sync_textures(rtx_ctx* c, MapUse use, bool renumbered, bool deformed) {
    SceneHost& H = c->host; rtx_ctx::Scene& S = c->scene;
    S.built.map_use = use;
    const bool active = use.any(), cut = use.cut(), nrm = use.nrm();       // (the UVs serve every group)
    int r;
    if (H.tex_dirty) {                                       // (a scene that never saw one of the three setters allocates nothing here)
        std::vector<TexDesc> desc(H.textures.size()); std::vector<uint32_t> pool;
        for (size_t i = 0; i < H.textures.size(); i++) {
            const TexHost& t = H.textures[i];
            desc[i] = TexDesc{(uint32_t)pool.size(), t.width, t.height, t.flags};
            pool.insert(pool.end(), t.rgba.begin(), t.rgba.end());
        }
        const size_t nm = S.mat_maps_nmat = H.mats128.size() / 32;
        std::vector<int32_t> ids(rtx_ctx::Scene::kMatMapRows * nm, -1);       // one row per slot the kernels read by material, -1 where the host's vector ends
        for (uint32_t s = 0; s < kMapSlotCount; s++)
            if (s != kMapOpacity) std::copy_n(H.maps[s].begin(), std::min(nm, H.maps[s].size()), ids.begin() + rtx_ctx::Scene::mat_map_row((MapSlot)s) * nm);
        if ((r = upload(c, S.d_tex_desc, desc)) || (r = upload(c, S.d_texels, pool)) || (r = upload(c, S.d_mat_maps, ids))) return r;
        if (!H.ess_rows) S.d_ess_tab.release();
        else if ((r = upload(c, S.d_ess_tab, H.ess_table))) return r;
        if (!S.d_tex_lut.p) { std::vector<float> lut; fill_tex_lut(lut); if ((r = upload(c, S.d_tex_lut, lut))) return r; }
        S.ntex = (uint32_t)desc.size();
    }
    if (active && (H.tex_dirty || renumbered || !S.tri_uv_valid)) {
        std::vector<float> uv; H.fill_tri_uv(uv);
        if ((r = upload(c, S.d_tri_uv, uv))) return r;
        S.tri_uv_valid = true;
    }
    if (!active && S.tri_uv_valid) { S.d_tri_uv.release(); S.tri_uv_valid = false; }       // (allocated only while a map is active)
    // alpha cut-outs: the opacity texture per GLOBAL triangle id — from maps[kMapOpacity], the material ids and the emitter test, numbered like tri_uv; never part of the leaf records
    if (cut && (H.tex_dirty || renumbered || !S.tri_cut_valid)) {
        std::vector<int32_t> tc; H.fill_tri_cut(tc);
        if ((r = upload(c, S.d_tri_cut, tc))) return r;
        S.tri_cut_valid = true;
    }
    if (!cut && S.tri_cut_valid) { S.d_tri_cut.release(); S.tri_cut_valid = false; }
    // normal maps: the object-space tangent record per GLOBAL triangle id, numbered like tri_uv — from the UVs and the meshes' current vertices, so a transform-only commit keeps it
    if (nrm && (H.tex_dirty || renumbered || deformed || !S.tri_tan_valid)) {
        std::vector<float> tt; H.fill_tri_tan(tt);
        if ((r = upload(c, S.d_tri_tan, tt))) return r;
        S.tri_tan_valid = true;
    }
    if (!nrm && S.tri_tan_valid) { S.d_tri_tan.release(); S.tri_tan_valid = false; }
    H.tex_dirty = false;
    return RTX_OK;
}

// The environment's tables follow the host's map (SceneHost::env): built in double on the host (rtx_env_host.cpp), uploaded; no kernel runs.  What the kernels see of
// them is set by finalise_scene.
static int sync_environment(rtx_ctx* c) {
    SceneHost& H = c->host; rtx_ctx::Scene& S = c->scene;
    S.built.env_active = H.env.n != 0;
    if (!H.env_dirty) return RTX_OK;
    H.env_dirty = false;
    if (!H.env.n) { S.d_env_tex.release(); S.d_env_marg.release(); S.d_env_cond.release(); S.env_total = 0.0; return RTX_OK; }
    EnvTables T; env_build_tables(H.env, T);
    int r;
    if ((r = upload(c, S.d_env_tex, T.texels4)) || (r = upload(c, S.d_env_marg, T.marginal)) || (r = upload(c, S.d_env_cond, T.conditional))) return r;
    S.env_total = T.total;
    return RTX_OK;
}

// a device array that only grows at its end: capacity in steps of 1.5 x, the `used` bytes survive a reallocation
static int grow_keep(rtx_ctx* c, DevBuf& b, size_t used, size_t need) {
    if (need <= b.bytes && b.p) return RTX_OK;
    DevBuf nb; HIPCHK(c, nb.ensure(std::max(need, b.bytes + b.bytes / 2)));
    if (used && b.p) HIPCHK(c, hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    b = std::move(nb);
    return RTX_OK;
}
// the device mesh pool follows the host's mesh list: the meshes added since the last commit are appended, the vertex ranges of the meshes named in pool_dirty (vertices
// replaced since the pool last saw them) are overwritten in place
static int sync_mesh_pool(rtx_ctx* c) {
    const SceneHost& H = c->host;
    if (H.meshes.size() < c->scene.pool_meshes) { c->scene.pool_meshes = 0; c->scene.pool_verts = c->scene.pool_idx = c->scene.pool_matids = 0; c->scene.pool_vert_base.clear(); c->scene.pool_idx_base.clear(); c->scene.pool_dirty.clear(); }     // (another scene: start over)
    const size_t had = c->scene.pool_meshes;
    size_t nv = c->scene.pool_verts, ni = c->scene.pool_idx;
    for (size_t m = c->scene.pool_meshes; m < H.meshes.size(); m++) { nv += H.meshes[m].verts.size() / 7; ni += H.meshes[m].idx.size(); }
    if (nv > 0xFFFFFFFFull || ni > 0xFFFFFFFFull) { c->err = "commit: more than 2^32 vertices or indices"; return RTX_ERR_INVALID; }
    int r;
    if ((r = grow_keep(c, c->scene.d_pool_verts, c->scene.pool_verts * 28, nv * 28))) return r;
    if ((r = grow_keep(c, c->scene.d_pool_idx, c->scene.pool_idx * 4, ni * 4))) return r;
    if ((r = grow_keep(c, c->scene.d_pool_matids, c->scene.pool_matids * 4, H.matids.size() * 4))) return r;
    for (size_t m = c->scene.pool_meshes; m < H.meshes.size(); m++) {
        const MeshHost& M = H.meshes[m];
        c->scene.pool_vert_base.push_back((uint32_t)c->scene.pool_verts); c->scene.pool_idx_base.push_back((uint32_t)c->scene.pool_idx);
        TO_DEVICE(c, (char*)c->scene.d_pool_verts.p + c->scene.pool_verts * 28, M.verts.data(), M.verts.size() * 4);
        TO_DEVICE(c, (char*)c->scene.d_pool_idx.p + c->scene.pool_idx * 4, M.idx.data(), M.idx.size() * 4);
        c->scene.pool_verts += M.verts.size() / 7; c->scene.pool_idx += M.idx.size();
    }
    c->scene.pool_meshes = H.meshes.size();
    if (H.matids.size() > c->scene.pool_matids) { TO_DEVICE(c, (char*)c->scene.d_pool_matids.p + c->scene.pool_matids * 4, H.matids.data() + c->scene.pool_matids, (H.matids.size() - c->scene.pool_matids) * 4); c->scene.pool_matids = H.matids.size(); }
    for (uint32_t m : c->scene.pool_dirty) {                 // (the vertex count of a mesh never changes: the range is the one it was appended to)
        if (m >= had) continue;                              // appended just now, with its current vertices
        const MeshHost& M = H.meshes[m];
        TO_DEVICE(c, (char*)c->scene.d_pool_verts.p + (size_t)c->scene.pool_vert_base[m] * 28, M.verts.data(), M.verts.size() * 4);
    }
    c->scene.pool_dirty.clear();
    return RTX_OK;
}
static FlatInst flat_inst(const rtx_ctx* c, size_t ii, uint32_t work_base) {
    const InstHost& in = c->host.insts[ii]; const MeshHost& M = c->host.meshes[in.mesh];
    return FlatInst{in.tri_base, (uint32_t)(M.idx.size() / 3), c->scene.pool_vert_base[in.mesh], c->scene.pool_idx_base[in.mesh], M.matid_base, work_base, (uint32_t)ii, 0u};
}
// the pool brought up to date; the per-instance ranges; then the flatten itself
static int flatten_on_device(rtx_ctx* c, uint32_t ntri) {
    const SceneHost& H = c->host;
    int r;
    if ((r = sync_mesh_pool(c))) return r;
    c->scene.h_flat.resize(H.insts.size());
    for (size_t ii = 0; ii < H.insts.size(); ii++) c->scene.h_flat[ii] = flat_inst(c, ii, H.insts[ii].tri_base);
    if ((r = upload(c, c->scene.d_flat_insts, c->scene.h_flat))) return r;
    HIPCHK(c, c->scene.d_objtris.ensure((size_t)ntri * 3 * sizeof(F4))); HIPCHK(c, c->scene.d_shade.ensure((size_t)ntri * sizeof(TriShade)));
    launch_flatten(c->stream, (const float*)c->scene.d_pool_verts.p, (const uint32_t*)c->scene.d_pool_idx.p, (const uint32_t*)c->scene.d_pool_matids.p, (uint32_t)H.matids.size(), (const FlatInst*)c->scene.d_flat_insts.p,
                   (uint32_t)c->scene.h_flat.size(), ntri, (F4*)c->scene.d_objtris.p, (TriShade*)c->scene.d_shade.p);
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}
// vertex-changing commit of a resident scene: object-space triangles and shade records of the instances of the changed meshes, re-derived in place (k_reflatten) from the
// pool — which a host-built scene gets here, on its first such commit
static int reflatten_dirty_meshes(rtx_ctx* c) {
    const SceneHost& H = c->host;
    int r;
    if ((r = sync_mesh_pool(c))) return r;
    c->scene.h_work.clear();
    uint64_t nitems = 0;
    for (size_t ii = 0; ii < H.insts.size(); ii++)
        if (H.mesh_is_dirty(H.insts[ii].mesh)) { c->scene.h_work.push_back(flat_inst(c, ii, (uint32_t)nitems)); nitems += c->scene.h_work.back().ntri; }
    if (!nitems) return RTX_OK;                              // (a changed mesh nobody instances)
    if ((r = upload(c, c->scene.d_work_insts, c->scene.h_work))) return r;
    launch_reflatten(c->stream, (const float*)c->scene.d_pool_verts.p, (const uint32_t*)c->scene.d_pool_idx.p, (const uint32_t*)c->scene.d_pool_matids.p, (uint32_t)H.matids.size(), (const FlatInst*)c->scene.d_work_insts.p,
                     (uint32_t)c->scene.h_work.size(), (uint32_t)nitems, (F4*)c->scene.d_objtris.p, (TriShade*)c->scene.d_shade.p);
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}

// instance visibility as committed (BuiltScene::inst_hidden), one word per instance, uploaded like inst_moved.  While nothing is hidden the refit kernels get no array at
// all: such scenes run exactly the launches, and upload exactly the bytes, they did before visibility existed
static int upload_hidden(rtx_ctx* c) {
    const BuiltScene& B = c->scene.built;
    return B.any_hidden ? upload(c, c->scene.d_inst_hidden, B.inst_hidden) : RTX_OK;
}
static const uint32_t* hidden_words(const rtx_ctx* c) { return c->scene.built.any_hidden ? (const uint32_t*)c->scene.d_inst_hidden.p : nullptr; }

// ---- tree quality (k_tree_cost, csrc/rtx_refit.hip) ----
static int full_refit(rtx_ctx* c) {              // world triangles from the object-space ones, every node quantised bottom-up, node_aabb filled: what the first transform-only commit after a build runs
    BuiltScene& B = c->scene.built;
    HIPCHK(c, c->scene.d_node_aabb.ensure((size_t)c->scene.n_nodes8 * 32));
    c->scene.h_one.assign(1, 0x3f800000u);                       // scale starts at 1.0 like the host's max(1, |coordinates|)
    int r;
    if ((r = upload(c, c->scene.d_scale, c->scene.h_one))) return r;
    if ((r = upload_hidden(c))) return r;
    launch_refit(c->stream, (Node8GPU*)c->scene.d_nodes.p, B.level_start8.data(), (uint32_t)B.level_start8.size() - 1, (TriGPU*)c->scene.d_tris.p, c->scene.n_tris8,
                 (const TriShade*)c->scene.d_shade.p, (const InstGPU*)c->scene.d_insts.p, (const F4*)c->scene.d_objtris.p, (F4*)c->scene.d_node_aabb.p, (uint32_t*)c->scene.d_scale.p, nullptr, nullptr, nullptr,
                 hidden_words(c));
    HIPCHK(c, hipGetLastError());
    c->scene.node_aabb_valid = true;
    return RTX_OK;
}
static int upload_objtris_once(rtx_ctx* c) {
    BuiltScene& B = c->scene.built;
    if (c->scene.objtris_uploaded) return RTX_OK;
    if (B.objtris.empty()) c->host.fill_objtris(B);             // scene came from a cache file: derive them from the meshes now
    int r = upload(c, c->scene.d_objtris, B.objtris);
    if (r == RTX_OK) c->scene.objtris_uploaded = true;
    return r;
}
static int enqueue_tree_cost(rtx_ctx* c, DevBuf& partial) {
    HIPCHK(c, partial.ensure((size_t)tree_cost_partials(c->scene.n_nodes8) * 4));
    launch_tree_cost(c->stream, (const F4*)c->scene.d_node_aabb.p, c->scene.n_nodes8, (float*)partial.p);
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}
static int read_tree_cost(rtx_ctx* c, const DevBuf& partial, double& out) {     // the partial sums added in index order, in double: the same bits whenever the boxes are the same
    std::vector<float> h(tree_cost_partials(c->scene.n_nodes8));
    TO_HOST(c, h.data(), partial.p, h.size() * 4);
    double sum = 0.0;
    for (size_t i = 0; i + 1 < h.size(); i++) sum += (double)h[i];
    out = (double)h.back() > 0.0 ? sum / (double)h.back() : 0.0;
    return RTX_OK;
}
// The baseline: the cost of the tree as its last build left it.  A GPU build records it behind its own full refit; a host-built tree has no float boxes on the device until its
// first refit, so it is taken when first needed — BEFORE the first vertex-changing commit touches the device, or at the first rtx_debug_tree_cost — from a full refit of the
// unchanged geometry (no commit without new vertices pays for it; transform-only refits that came earlier are part of that baseline).  *refitted: the nodes were re-quantised
static int ensure_cost_baseline(rtx_ctx* c, bool* refitted) {
    if (c->scene.cost_base_state) return RTX_OK;
    int r;
    if (!c->scene.node_aabb_valid) {
        if ((r = upload_objtris_once(c))) return r;
        if ((r = full_refit(c))) return r;
        if (refitted) *refitted = true;
    }
    if ((r = enqueue_tree_cost(c, c->scene.d_cost_base))) return r;
    c->scene.cost_base_state = 1;
    return RTX_OK;
}
static bool gpu_refittable(const rtx_ctx* c) {
    const BuiltScene& B = c->scene.built;
    return c->scene.device_scene_valid && B.small_nrec == 0 && c->scene.n_nodes8 != 0 && B.level_start8.size() >= 2;
}
static int refresh_wide_nodes(rtx_ctx* c);
// probe_anyhit_order (csrc/rtx_scene_host.cpp) for a tree the host holds no mirror of (RTX_OPT_GPU_BUILD): the same 2 048 NEE-like segments — a point on a random triangle to a
// CDF-sampled point on a light —, traced ON THE DEVICE in the three visiting orders by the counting form of the any-hit traversal, judged by the same cost model
static int probe_anyhit_order_on_device(rtx_ctx* c, uint32_t& best_out) {
    const BuiltScene& B = c->scene.built;
    best_out = 0u;
    const uint32_t nt = B.built_tris;
    if (B.lights.empty() || !nt || c->scene.h_flat.empty()) return RTX_OK;
    auto h32 = [](uint32_t a, uint32_t b) { uint32_t h = a * 0x9E3779B1u ^ (b + 0x7F4A7C15u) * 0x85EBCA77u; h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15; return h; };
    auto r01 = [&](uint32_t a, uint32_t b) { return (float)(h32(a, b) >> 8) * (1.0f / 16777216.0f); };
    std::vector<float> rays; rays.reserve(2048 * 8);
    for (uint32_t i = 0; i < 2048u; i++) {
        const uint32_t g = h32(i, 1u) % nt;
        size_t ii = (size_t)(std::upper_bound(c->scene.h_flat.begin(), c->scene.h_flat.end(), g, [](uint32_t v, const FlatInst& F) { return v < F.tri_base; }) - c->scene.h_flat.begin()) - 1;      // the last instance starting at or before g
        const float* M = B.insts[ii].o2w; const MeshHost& mesh = c->host.meshes[c->host.insts[ii].mesh];
        const uint32_t t = g - c->scene.h_flat[ii].tri_base;
        f3 w[3]; for (int k = 0; k < 3; k++) { const float* o = &mesh.verts[(size_t)mesh.idx[(size_t)t * 3 + k] * 7]; w[k] = xform_point(M, mk3(o[0], o[1], o[2])); }
        const f3 e1 = w[1] - w[0], e2 = w[2] - w[0];
        float u = r01(i, 2u), v = r01(i, 3u); if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
        const f3 p = mk3(w[0].x + u * e1.x + v * e2.x, w[0].y + u * e1.y + v * e2.y, w[0].z + u * e1.z + v * e2.z);
        f3 n = normalize(cross(e1, e2));
        const float xi = r01(i, 4u);
        size_t li = 0; while (li + 1 < B.lights.size() && B.lights[li].cdf < xi) li++;
        const LightGPU& Lg = B.lights[li];
        float a = r01(i, 5u), b = r01(i, 6u); if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
        const f3 lp = mk3(Lg.xv[0] + a * (Lg.yv[0] - Lg.xv[0]) + b * (Lg.zv[0] - Lg.xv[0]), Lg.xv[1] + a * (Lg.yv[1] - Lg.xv[1]) + b * (Lg.zv[1] - Lg.xv[1]), Lg.xv[2] + a * (Lg.yv[2] - Lg.xv[2]) + b * (Lg.zv[2] - Lg.xv[2]));
        f3 dir = lp - p;
        if (dot(n, dir) < 0.0f) n = mk3(-n.x, -n.y, -n.z);
        const f3 org = mk3(p.x + kSBias * n.x, p.y + kSBias * n.y, p.z + kSBias * n.z);
        dir = lp - org;
        const float dist = length(dir);
        if (!(dist > 10.0f * kSBias)) continue;
        const float r8[8] = {org.x, org.y, org.z, 0.5f * kSBias, dir.x / dist, dir.y / dist, dir.z / dist, dist - 5.0f * kSBias};
        rays.insert(rays.end(), r8, r8 + 8);
    }
    const uint32_t n = (uint32_t)(rays.size() / 8);
    if (!n) return RTX_OK;
    DevBuf d_rays, d_out;
    HIPCHK(c, d_rays.ensure((size_t)n * 32)); HIPCHK(c, d_out.ensure((size_t)n * 16 * 3));
    TO_DEVICE(c, d_rays.p, rays.data(), (size_t)n * 32);
    for (uint32_t ord = 0; ord < 3u; ord++) { DevScene sc = c->dsc; sc.any_order = ord; launch_dbg_trace(c->stream, sc, (const F4*)d_rays.p, n, 3, (F4*)d_out.p + (size_t)ord * n); }
    HIPCHK(c, hipGetLastError());
    std::vector<float> h((size_t)n * 4 * 3);
    TO_HOST(c, h.data(), d_out.p, h.size() * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    double cost[3] = {0.0, 0.0, 0.0};
    for (uint32_t ord = 0; ord < 3u; ord++) for (uint32_t i = 0; i < n; i++) { const float* q = &h[((size_t)ord * n + i) * 4]; cost[ord] += (double)q[1] * (205.0 * 64.0 / 47.0) + (double)q[2] * (70.0 * 64.0 / 24.0); }
    for (uint32_t ord = 1; ord < 3u; ord++) if (cost[ord] < 0.95 * cost[0] && cost[ord] < cost[best_out]) best_out = ord;
    return RTX_OK;
}

// Transform- or vertex-only commit of a resident scene: refit ON THE GPU — the kernels re-derive the world triangles and re-quantise the wide nodes bottom-up; the host only
// re-derives the instance matrices and the light list.  New vertices (rtx_update_mesh_vertices): the changed meshes go to the pool and k_reflatten re-derives the object-space
// triangles and shade records of their instances first; refresh_transforms has flagged those instances like moved ones, so the same partial refit follows.
static int refit_resident(rtx_ctx* c, bool deform) {
    BuiltScene& B = c->scene.built;
    int r;
    if (deform && (r = ensure_cost_baseline(c, nullptr))) return r;      // (while the device still holds the geometry of the last commit)
    const bool mats_changed = c->host.mats_dirty;
    if (!c->host.refresh_transforms(B)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    if (mats_changed && (r = upload(c, c->scene.d_mats, B.mats))) return r;      // rtx_set_materials on a resident scene: new table beside the new light list
    if ((r = upload(c, c->scene.d_insts, B.insts))) return r;
    if ((r = upload_lights(c))) return r;
    if ((r = upload_objtris_once(c))) return r;
    if (deform) {
        if ((r = reflatten_dirty_meshes(c))) return r;
        // the host's copies of the per-triangle records now describe the old vertices.  The stale-mirror rule: nothing reads them again — the object-space triangles are dropped
        // (fill_objtris re-derives them from the meshes if they are ever uploaded again), the shade records stay for their count only and rtx_save_scene_cache refuses
        if (!c->scene.dev_built) { B.objtris.clear(); B.objtris.shrink_to_fit(); c->scene.host_mirror_stale = true; }
    }
    HIPCHK(c, c->scene.d_node_aabb.ensure((size_t)c->scene.n_nodes8 * 32));
    // the first refit after a build is a full one (it fills node_aabb); later ones touch the moved instances only, unless every instance moved anyway
    size_t nmoved = 0; for (uint32_t m : B.inst_moved) nmoved += m;
    const bool partial = c->opt.partial_refit && c->scene.node_aabb_valid && B.inst_moved.size() == B.insts.size() && nmoved < B.insts.size();
    if (!partial) return full_refit(c);
    if ((r = upload(c, c->scene.d_inst_moved, B.inst_moved))) return r;
    if ((r = upload_hidden(c))) return r;
    HIPCHK(c, c->scene.d_tri_dirty.ensure(c->scene.n_tris8)); HIPCHK(c, c->scene.d_node_dirty.ensure(c->scene.n_nodes8));
    launch_refit(c->stream, (Node8GPU*)c->scene.d_nodes.p, B.level_start8.data(), (uint32_t)B.level_start8.size() - 1, (TriGPU*)c->scene.d_tris.p, c->scene.n_tris8,
                 (const TriShade*)c->scene.d_shade.p, (const InstGPU*)c->scene.d_insts.p, (const F4*)c->scene.d_objtris.p, (F4*)c->scene.d_node_aabb.p, (uint32_t*)c->scene.d_scale.p,
                 (const uint32_t*)c->scene.d_inst_moved.p, (uint8_t*)c->scene.d_tri_dirty.p, (uint8_t*)c->scene.d_node_dirty.p, hidden_words(c));
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}

// Anything else: host build (or host refit — topo_dirty == false: from the meshes as they are now, new vertices included) + upload, or the build on the device
static int build_and_upload(rtx_ctx* c) {
    BuiltScene& B = c->scene.built;
    int r;
    c->scene.device_scene_valid = false; c->scene.objtris_uploaded = false; c->scene.node_aabb_valid = false; c->scene.host_mirror_stale = false;
    size_t ntri_all = 0; for (const InstHost& in : c->host.insts) ntri_all += c->host.meshes[in.mesh].idx.size() / 3;
    // RTX_OPT_GPU_BUILD: the tree on the device (csrc/rtx_build.hip).  Not for tiny scenes (their pre-test records are built from the host tree's leaf order) nor with
    // spatial splits (a host-builder feature); there the host builds as before.
    const bool on_gpu = c->opt.gpu_build && ntri_all > 4096u && c->host.bvh.split_alpha <= 0.0;
    if (!(on_gpu ? c->host.prepare_device_build(B) : c->host.build(B))) { c->err = c->host.err; return RTX_ERR_INVALID; }
    if (!on_gpu) {
        if ((r = upload_built(c))) return r;
        // The host builder knows nothing of visibility: its tree, boxes and triangle records are those of all instances.  With a hidden instance — and only then — the
        // hand-over ends like the GPU build's: ONE full pass of the refit kernels, which writes the never-hit records and takes the hidden triangles out of the boxes.
        // (This holds for the host refit of RTX_OPT_GPU_REFIT 0 as well, and for a tiny scene, which SceneHost::build sends through the general path while anything is hidden.)
        if (B.any_hidden && c->scene.n_nodes8 && B.level_start8.size() >= 2) {
            if ((r = upload_objtris_once(c))) return r;
            if ((r = full_refit(c))) return r;
            TO_HOST(c, &c->scene.root8, c->scene.d_nodes.p, sizeof(Node8GPU));
        }
        return RTX_OK;
    }
    const uint32_t nt = B.built_tris;
    if ((r = upload(c, c->scene.d_mats, B.mats))) return r;
    if ((r = upload(c, c->scene.d_insts, B.insts))) return r;
    if ((r = upload_lights(c))) return r;
    if ((r = flatten_on_device(c, nt))) return r; c->scene.objtris_uploaded = true;          // object-space triangles + shade records, from the resident meshes
    for (DevBuf* b : {&c->scene.d_small, &c->scene.d_small_tris, &c->scene.d_small_poly, &c->scene.d_small_slabs}) HIPCHK(c, b->ensure(16));
    HIPCHK(c, c->scene.d_tris.ensure((size_t)nt * sizeof(TriGPU)));
    if (!c->scene.builder) c->scene.builder.reset(new GpuBvhBuilder());
    BvhBuildOptions bo = c->host.bvh; if (bo.ploc_radius <= 0) bo.ploc_radius = 16;
    const std::string e = c->scene.builder->build(c->stream, (const F4*)c->scene.d_objtris.p, (const TriShade*)c->scene.d_shade.p, (const InstGPU*)c->scene.d_insts.p, nt, bo, (TriGPU*)c->scene.d_tris.p, c->scene.build_info);
    if (!e.empty()) { c->err = e; return RTX_ERR_HIP; }
    const GpuBuildResult& G = c->scene.build_info;
    HIPCHK(c, c->scene.d_nodes.ensure((size_t)G.nnodes8 * sizeof(Node8GPU)));
    HIPCHK(c, hipMemcpyAsync(c->scene.d_nodes.p, c->scene.builder->nodes(), (size_t)G.nnodes8 * sizeof(Node8GPU), hipMemcpyDeviceToDevice, c->stream));
    c->scene.n_nodes8 = G.nnodes8; c->scene.n_tris8 = G.ntris8; c->scene.dev_built = true; B.bvh_pad = 2e-6f * G.scale;
    B.level_start8 = G.level_start8; B.stack8 = G.stack8;
    // the boxes: a FULL refit — world triangles from the object-space ones, every node quantised bottom-up (what a transform-only commit runs)
    if ((r = full_refit(c))) return r;
    if (c->scene.n_nodes8) { if ((r = enqueue_tree_cost(c, c->scene.d_cost_base))) return r; c->scene.cost_base_state = 1; }     // the baseline of RTX_OPT_DEFORM_REBUILD: one small launch, read when asked for
    TO_HOST(c, &c->scene.root8, c->scene.d_nodes.p, sizeof(Node8GPU));
    if (getenv("RTX_BUILD_TIMES")) fprintf(stderr, "[build] GPU: prims %.2f ms, sort %.2f ms, PLOC %.2f ms (%u rounds -> %u clusters), top on the host %.2f ms, layout %.2f ms: %u wide nodes, stack %u\n",
                                           G.ms_prims, G.ms_sort, G.ms_ploc, G.ploc_iterations, G.clusters_top, G.ms_top_host, G.ms_layout, G.nnodes8, G.stack8);
    return RTX_OK;
}

int rtx_commit_scene(rtx_ctx* c) {
    BIND(c);
    // rtx_update_mesh_vertices since the last commit: topology stays, so this commit REFITS (BottomLevelASGenerator.cpp:185-209, updateOnly) — unless RTX_OPT_DEFORM_REBUILD
    // says rebuild (1), or (N >= 2) the refitted tree has degraded past N % of its cost after the last build, which the same commit then answers with a rebuild
    const bool deform = !c->host.dirty_meshes.empty();
    for (uint32_t m : c->host.dirty_meshes)
        if (m < c->scene.pool_meshes && std::find(c->scene.pool_dirty.begin(), c->scene.pool_dirty.end(), m) == c->scene.pool_dirty.end()) c->scene.pool_dirty.push_back(m);
    if (deform && c->opt.deform_rebuild == 1) c->host.topo_dirty = true;
    if (c->host.topo_dirty || c->host.mats_dirty || !c->scene.committed_once)      // (a transform-only commit changes neither the ids nor the table: not 11 M comparisons per frame)
        for (size_t i = 0; i < c->host.matids.size(); i++)
            if (c->host.matids[i] >= c->host.mats128.size() / 32) { c->err = "commit: material id out of range"; return RTX_ERR_INVALID; }
    c->scene.committed_once = true;
    int r;
    // On the GPU: a scene that is already resident and not a tiny one (whose pre-test records depend on world positions).
    // a tiny scene leaves its pre-test records for the general path while a texture map is active and returns to them afterwards: the commit that crosses that line rebuilds
    const MapUse use = c->host.map_use();                  // the map groups active from this commit on (one pass over the triangles; nothing below changes what it reads)
    {   size_t ntri_all = 0; for (const InstHost& in : c->host.insts) ntri_all += c->host.meshes[in.mesh].idx.size() / 3;
        if (c->host.tex_dirty && ntri_all <= kSmallSceneMaxTris && use != c->scene.built.map_use) c->host.topo_dirty = true;
        // ... and so it does while an environment is bound
        if (c->host.env_dirty && ntri_all <= kSmallSceneMaxTris && (c->host.env.n != 0) != c->scene.built.env_active) c->host.topo_dirty = true; }
    bool build = !(c->opt.gpu_refit && gpu_refittable(c) && !c->host.topo_dirty);
    // a tiny scene whose last instance was just shown again returns to its pre-test records: a host refit (SceneHost::build derives them from world positions)
    const BuiltScene& B0 = c->scene.built;
    if (!build && !c->scene.dev_built && !B0.leaf_order.empty() && B0.leaf_order.size() <= kSmallSceneMaxTris && B0.any_hidden && !c->host.any_hidden()) build = true;
    bool flipped = false;                                  // a resident scene's visibility differs from the caller's
    for (size_t ii = 0; ii < c->host.insts.size() && !flipped; ii++) flipped = (ii < B0.inst_hidden.size() && B0.inst_hidden[ii] != 0u) != c->host.is_hidden(ii);
    // only UVs, textures or map ids changed on a resident general scene: tables are uploaded, nothing is refitted (rtx_stats.bvh_refits and the tree stay)
    // ... and likewise when only the environment changed
    const bool tex_only = !build && (c->host.tex_dirty || c->host.env_dirty) && c->host.only_maps_changed(B0);
    // ... except that, while an emission map is active on an emitter or was at the previous commit, the light list follows the texels: rebuilt on the host, uploaded
    if (tex_only && c->host.tex_dirty && (B0.map_use.emi() || use.emi())) {
        c->host.build_lights(c->scene.built);
        if ((r = upload_lights(c))) return r;
    }
    const bool probe = (build || !flipped) && !tex_only;   // the any-hit order is a property of the tree and the lights' whereabouts: not re-probed because something was hidden or shown
    if (!build && !tex_only) {
        if ((r = refit_resident(c, deform))) return r;
        c->scene.cost_now_state = 0;
        if (deform && c->opt.deform_rebuild >= 2) {
            double cost[2];
            if ((r = tree_costs(c, cost))) return r;
            if (cost[0] * 100.0 > cost[1] * (double)c->opt.deform_rebuild) { c->host.topo_dirty = true; build = true; }
        }
    }
    if (build) {
        c->scene.cost_base_state = c->scene.cost_now_state = 0;
        if ((r = build_and_upload(c))) return r;
    }
    c->host.dirty_meshes.clear();
    if ((r = sync_textures(c, use, build, deform))) return r;
    if ((r = sync_environment(c))) return r;
    r = finalise_scene(c);
    if (r == RTX_OK && c->scene.dev_built && c->scene.n_nodes8 && probe) {          // the visiting order of any-hit rays, probed on the device (the host probe replays its mirror of the tree)
        uint32_t best = 0;
        if ((r = probe_anyhit_order_on_device(c, best))) return r;
        c->scene.built.any_order = best;
        if (c->opt.any_order_opt < 0) c->dsc.any_order = best;
    }
    return r;
}

// the binary scene cache.  Save = the committed scene (inputs + everything rtx_commit_scene derived); load = replace the
// context's scene by the file's and upload it, instead of rtx_set_materials / rtx_add_mesh / rtx_add_instance / rtx_commit_scene.
int rtx_save_scene_cache(rtx_ctx* c, const char* path) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->committed) { c->err = "save_scene_cache: scene not committed"; return RTX_ERR_STATE; }
    if (c->scene.host_mirror_stale) { c->err = "save_scene_cache: the per-triangle records were re-derived on the GPU after rtx_update_mesh_vertices and the host holds no current copy; commit with RTX_OPT_DEFORM_REBUILD 1 (host builder) to save a cache"; return RTX_ERR_STATE; }
    if (c->scene.built.any_hidden) { c->err = "save_scene_cache: an instance is hidden (rtx_set_instance_visible): the device's boxes and triangle records leave it out and the file format holds no visibility; show every instance and commit to save a cache"; return RTX_ERR_STATE; }
    if (c->host.env.n) { c->err = "save_scene_cache: an environment is bound (rtx_set_environment) and the file format holds no environment; clear it and commit to save a cache"; return RTX_ERR_STATE; }
    for (uint32_t s = 0; s < kMapSlotCount; s++)
        if (c->host.any_bound((MapSlot)s)) { c->err = std::string("save_scene_cache: a material has a texture map (rtx_set_material_map, ") + kMapSlots[s].name + ") and the file format holds no texels; unmap every material and commit to save a cache"; return RTX_ERR_STATE; }
    if (c->scene.dev_built) { c->err = "save_scene_cache: the tree was built on the GPU (RTX_OPT_GPU_BUILD) and has no host mirror; commit with the host builder to save a cache"; return RTX_ERR_STATE; }
    if (!save_scene_cache(c->host, c->scene.built, path, c->err)) return RTX_ERR_INVALID;
    return RTX_OK;
}
int rtx_load_scene_cache(rtx_ctx* c, const char* path) {
    BIND(c);
    if (!load_scene_cache(path, c->host, c->scene.built, c->err)) return RTX_ERR_INVALID;     // on failure the previous scene is untouched
    c->committed = false; c->scene.device_scene_valid = false; c->scene.objtris_uploaded = false; c->scene.node_aabb_valid = false;
    c->scene.host_mirror_stale = false; c->scene.cost_base_state = c->scene.cost_now_state = 0;
    c->scene.pool_meshes = 0; c->scene.pool_verts = c->scene.pool_idx = c->scene.pool_matids = 0; c->scene.pool_vert_base.clear(); c->scene.pool_idx_base.clear(); c->scene.pool_dirty.clear();     // (another scene)
    int r = upload_built(c);
    if (r) return r;
    c->host.tex_dirty = true;                  // (another scene: no textures, no maps)
    if ((r = sync_textures(c, c->host.map_use(), true, false))) return r;
    c->host.env = EnvHost{}; c->host.env_dirty = true;      // (another scene: no environment)
    if ((r = sync_environment(c))) return r;
    return finalise_scene(c);
}

static int refresh_wide_nodes(rtx_ctx* c) {        // the one-node-per-line copy follows the nodes (after every build / refit)
    if (!c->scene.wide_nodes || !c->scene.n_nodes8) return RTX_OK;
    HIPCHK(c, c->scene.d_nodes_wide.ensure((size_t)c->scene.n_nodes8 * 128));
    HIPCHK(c, hipMemcpy2DAsync(c->scene.d_nodes_wide.p, 128, c->scene.d_nodes.p, sizeof(Node8GPU), sizeof(Node8GPU), c->scene.n_nodes8, hipMemcpyDeviceToDevice, c->stream));
    return RTX_OK;
}
static int finalise_scene(rtx_ctx* c) {
    BuiltScene& B = c->scene.built;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->scene.device_scene_valid = true;
    DevScene& s = c->dsc;
    s.nodes = (const Node8GPU*)c->scene.d_nodes.p; s.nnodes = c->scene.n_nodes8;
    s.nodes_f = (const F4*)c->scene.d_nodes.p; s.node_v4 = 5u;
    // RTX_OPT_NODE_STRIDE: a second copy of the nodes with ONE node per 128-B line (80-B nodes at an 80-B stride straddle a line in 4 of 8 positions: 1.5 lines per visit),
    // refreshed after every build / refit (stream order: before any frame).  Auto: made for trees of more than 16 MB, and fetched by the path tracer's closest-hit launches of
    // bounces >= 1 only — incoherent rays on a tree far larger than L2 gain (street scene, 3.8 M triangles: k_trace_closest -2.4 %), coherent ones (camera rays, ReSTIR's
    // stages) and the any-hit kernel like neighbours sharing lines (+1 %), small trees do not care (profiles/r04_node_stride_ab.md).  128: every traversal fetches the wide copy.
    c->scene.wide_nodes = s.nnodes && (c->opt.node_stride == 128 || (c->opt.node_stride == 0 && (size_t)s.nnodes * sizeof(Node8GPU) > ((size_t)16 << 20)));
    { const int rw = refresh_wide_nodes(c); if (rw) return rw; }
    if (c->scene.wide_nodes && c->opt.node_stride == 128) { s.nodes_f = (const F4*)c->scene.d_nodes_wide.p; s.node_v4 = 8u; }
    s.tris = (const TriGPU*)c->scene.d_tris.p; s.ntris = c->scene.n_tris8;
    s.shade = (const TriShade*)c->scene.d_shade.p;
    s.small = (const SmallRecPair*)c->scene.d_small.p; s.small_tris = (const TriGPU*)c->scene.d_small_tris.p; s.small_poly = (const F4*)c->scene.d_small_poly.p; s.small_slabs = (const SmallSlabPair*)c->scene.d_small_slabs.p; s.small_cm = B.small_cm; s.small_delta = B.small_delta;
    s.mats = (const MatGPU*)c->scene.d_mats.p; s.nmat = (uint32_t)B.mats.size();
    s.insts = (const InstGPU*)c->scene.d_insts.p; s.ninst = (uint32_t)B.insts.size();
    s.lights = (const LightGPU*)c->scene.d_lights.p; s.nlights = (uint32_t)B.lights.size(); s.cdf = (const float*)c->scene.d_cdf.p;
    s.total_weight = B.total_weight;
    const MapUse use = B.map_use;
    if (use.emi() && !(B.total_weight > 0.0f)) s.nlights = 0;     // emission maps: every map black, no emitter has weight — the renderer has no light list (rtx_stats.lights and rtx_get_lights keep the count)
    // texture maps: the sampler's tables whenever there are textures; UVs and map ids only while a map is active (then k_shade<.., TEX> runs, rtx_render.hip)
    s.tex_desc = (const TexDesc*)c->scene.d_tex_desc.p; s.ntex = c->scene.ntex; s.texels = (const uint32_t*)c->scene.d_texels.p; s.tex_lut = (const float*)c->scene.d_tex_lut.p;
    // environment lighting: env_n says one is bound (the separate default kernels run), env_tex that it has weight (k_shade<.., ENV> runs)
    s.env_n = c->host.env.n; s.env_flags = c->host.env.flags; memcpy(s.env_rot, c->host.env.rot, sizeof(s.env_rot));
    const bool env_lit = s.env_n && c->scene.env_total > 0.0;
    s.env_tex = env_lit ? (const F4*)c->scene.d_env_tex.p : nullptr; s.env_marg = env_lit ? (const float*)c->scene.d_env_marg.p : nullptr; s.env_cond = env_lit ? (const float*)c->scene.d_env_cond.p : nullptr;
    // (a scene with cut-outs and no diffuse map: k_shade<.., TEX> runs all the same, selected by tri_uv, and reads a map_kd table of -1s — every material keeps its own Kd)
    // the per-material id rows: null unless the slot's group is active, except that map_kd is set whenever any group is
    const rtx_ctx::Scene& S = c->scene;
    s.tri_uv = use.any() ? (const float*)S.d_tri_uv.p : nullptr; s.map_kd = use.any() ? S.mat_maps(kMapKd) : nullptr;
    s.tri_cut = use.cut() ? (const int32_t*)S.d_tri_cut.p : nullptr;
    s.map_ks = use.spc() ? S.mat_maps(kMapKs) : nullptr; s.map_pr = use.spc() ? S.mat_maps(kMapPr) : nullptr; s.map_pm = use.spc() ? S.mat_maps(kMapPm) : nullptr;
    s.ess_tab = (use.spc() && c->host.ess_rows) ? (const float*)S.d_ess_tab.p : nullptr; s.ess_rows = s.ess_tab ? c->host.ess_rows : 0u;
    s.map_ke = use.emi() ? S.mat_maps(kMapKe) : nullptr; s.emi_q = use.emi() ? (const float*)S.d_emi_q.p : nullptr;
    s.tri_tan = use.nrm() ? (const float*)S.d_tri_tan.p : nullptr; s.map_nrm = use.nrm() ? S.mat_maps(kMapNormal) : nullptr;
    // LDS budget per workgroup: stack + top of tree + first triangles, kept <= 64 KiB
    // exact bound of the 8-wide tree, no slack: a level adds ONE entry (the rest of its hit siblings) and only where a node has >= 2 internal
    // children (collapse_bvh8: need[]); a pop precedes every descent from an exhausted group.  Each entry costs 1.5 KB of LDS per workgroup (6 B per lane: kStackEntryBytes), and
    // LDS decides how many workgroups live on a CU: two entries of slack cost C3 2.3 % (5 instead of 6 workgroups) and C5 1.3 %.
    s.stack_depth = B.stack8;
    // RTX_OPT_STACK_CAP (round 5): LDS pays for `stack_cap` entries at most; a tree whose exact bound is deeper keeps its remaining entries in per-lane columns in global memory
    // (StackLdsT<true>, rtx_traverse.hpp).  The bound is reached by a handful of rays, the LDS it costs is paid by every workgroup as staged nodes (73 at a bound of 9, 44 at 11,
    // 24 at 12).  Measured (tools/frame_ms.py, hard street scene): GPU-built tree, bound 12: 40.2 -> 39.4 ms with a cap of 9; host-built, bound 11: 39.75 -> 40.0; the
    // street stand-in, bound 10: 30.2 -> 30.4 — the overflow test on every push and pop costs about what 30 more staged nodes bring, so the default cap of 11 only catches the
    // deep trees, for which it is also the difference between running and "BVH too deep for the LDS traversal stack".  Columns: 2^22 lanes (16 384 workgroups: more than any
    // launch of this library keeps resident) x 8 B per entry beyond the cap.
    s.stack_ovf = nullptr; s.stack_ovf_stride = 0;
    if (c->opt.stack_cap && B.stack8 > c->opt.stack_cap && B.stack8 <= 30) {
        const uint32_t stride = 1u << 22;
        HIPCHK(c, c->scene.d_stack_ovf.ensure((size_t)(B.stack8 - c->opt.stack_cap) * stride * 8));
        s.stack_depth = c->opt.stack_cap; s.stack_ovf = (unsigned long long*)c->scene.d_stack_ovf.p; s.stack_ovf_stride = stride;
    }
    s.stack_private = c->opt.stack_private == 1 ? 1u : 0u;    // 1 (private / scratch) is a tuning knob; it measured slower than the LDS column
    if (s.stack_depth > 30) { c->err = "commit: BVH too deep for the traversal stack (more than 30 levels of 8-wide nodes with two or more internal children)"; return RTX_ERR_INVALID; }
    // LDS per workgroup = traversal stack (6 B per entry and lane) + top of the tree (+ all triangles of a small scene), <= 64 KiB.
    const size_t stack_bytes = (size_t)s.stack_depth * 256 * kStackEntryBytes;
    const size_t hard = 64 * 1024;
    size_t budget = hard > stack_bytes ? hard - stack_bytes : 0;
    uint32_t want_nodes;
    if (c->opt.lds_nodes_opt >= 0) want_nodes = (uint32_t)c->opt.lds_nodes_opt;
    else {
        want_nodes = 73;                                   // root + 8 + 64: the first three levels of the wide tree; trimmed below for occupancy
    }
    s.lds_nodes = std::min<uint32_t>(std::min<uint32_t>(want_nodes, s.nnodes), (uint32_t)(budget / 80));
    budget -= (size_t)s.lds_nodes * 80;
    uint32_t want_tris = s.ntris <= 256 ? s.ntris : 0u;                    // triangles only when ALL of them fit
    s.lds_tris = (size_t)want_tris * 48 <= budget ? want_tris : 0u;
    s.nsmall = 0; s.nsmall_occ = 0;
    {   // grid of RTX_OPT_OCTANT_SORT 3 over the root's box: 8 bits handed to the axes one at a time, always to the axis whose cells are longest
        float ext[3] = {1.0f, 1.0f, 1.0f}; uint32_t bits[3] = {0, 0, 0};
        s.cell_o[0] = s.cell_o[1] = s.cell_o[2] = 0.0f;
        if (c->scene.n_nodes8) {
            const Node8GPU& R0 = c->scene.root8;
            s.cell_o[0] = R0.px; s.cell_o[1] = R0.py; s.cell_o[2] = R0.pz;
            for (int a = 0; a < 3; a++) ext[a] = std::max(1e-20f, 255.0f * std::ldexp(1.0f, (int)((R0.e_imask >> (8 * a)) & 0xffu) - 127));
        }
        for (int k = 0; k < 8; k++) { int best = 0; for (int a = 1; a < 3; a++) if (ext[a] / (float)(1u << bits[a]) > ext[best] / (float)(1u << bits[best])) best = a; bits[best]++; }
        for (int a = 0; a < 3; a++) s.cell_s[a] = (float)(1u << bits[a]) / ext[a];
        s.cell_bits = bits[0] | (bits[1] << 4) | (bits[2] << 8);
    }
    options_to_scene(c, true);                             // (the any-hit order included: this commits the scene)
    if (c->opt.small_scene && B.small_nrec && B.small_tris.size() * 48 <= budget + (size_t)s.lds_tris * 48) {
        s.nsmall = B.small_nrec; s.nsmall_occ = B.small_nocc; s.lds_tris = (uint32_t)B.small_tris.size();   // LDS holds the records' triangles instead of the leaf-ordered ones
    }
    if (trace_lds_bytes(s) > 64 * 1024) { c->err = "commit: BVH too deep for the LDS traversal stack"; return RTX_ERR_INVALID; }
    // Staged nodes vs workgroups per CU.  The persistent traversal kernels are limited by LDS (160 KB per CU), and they gain from every workgroup
    // (`k_trace_shadow` C3: 12.8 -> 12.0 ms for one more) more than from nodes in LDS.  So: the workgroup count that root + 8 nodes alone would reach,
    // and then as many nodes as fit beside it.  Measured per frame: C3 41.5 ms with 9 nodes, 40.9 with 50 (eight workgroups either way,
    // `k_trace_closest` 21.9 -> 21.4 ms), 41.3 with 57-73 (seven); C5 40.4 ms with 73 nodes, 38.6 with 9, 38.3 with 31.  RTX_DEBUG_LDS=1 prints the choice.
    // (LDS is granted in 512-B granules, which the runtime's occupancy query does not count: 33 nodes on C5 "fit" seven workgroups by its answer and
    // ran like six.  Hence the model below, with the query only as the upper bound the registers set.)
    if (c->opt.lds_nodes_opt < 0 && !s.nsmall && s.lds_nodes > 9u) {
        auto fit = [&](uint32_t nodes) { DevScene t = s; t.lds_nodes = nodes; return (160u * 1024u) / (uint32_t)((trace_lds_bytes(t) + 64 + 1023) & ~(size_t)1023); };      // (1-KB granule: what round 4's sweeps fit, profiles/r04_lds_closest_ab.md)
        DevScene t9 = s; t9.lds_nodes = 9;
        const int by_regs = trace_workgroups_per_cu(t9);
        const uint32_t target = std::min<uint32_t>(fit(9), by_regs > 0 ? (uint32_t)by_regs : 8u);
        while (s.lds_nodes > 9u && fit(s.lds_nodes) < target) s.lds_nodes--;
        if (getenv("RTX_DEBUG_LDS")) fprintf(stderr, "[rtx] stack_depth %u workgroups per CU %u, %u nodes staged, %zu B of LDS\n", s.stack_depth, target, s.lds_nodes, trace_lds_bytes(s));
    }
    pick_lds_closest(c);
    c->stats.bvh_refits = B.refit_count; c->stats.bvh_nodes = s.nnodes; c->stats.triangles = B.shade.empty() ? B.built_tris : (uint32_t)B.shade.size(); c->stats.bvh_refs = s.ntris; c->stats.lights = (uint32_t)B.lights.size(); c->stats.materials = s.nmat;
    c->committed = true;
    return RTX_OK;
}

}  // extern "C"

int tree_costs(rtx_ctx* c, double out2[2]) {
    if (!gpu_refittable(c) || c->host.topo_dirty) { c->err = "tree_cost: this tree is not refitted on the GPU (a tiny scene with pre-test records, or no tree)"; return RTX_ERR_STATE; }
    int r; bool refitted = false;
    if ((r = ensure_cost_baseline(c, &refitted))) return r;
    if (refitted && (r = refresh_wide_nodes(c))) return r;          // (a re-quantised tree: the one-node-per-line copy follows, as after every refit)
    if (c->scene.cost_base_state == 1) { if ((r = read_tree_cost(c, c->scene.d_cost_base, c->scene.cost_base))) return r; c->scene.cost_base_state = 2; }
    if (c->scene.cost_now_state == 0) { if ((r = enqueue_tree_cost(c, c->scene.d_cost_now))) return r; c->scene.cost_now_state = 1; }
    if (c->scene.cost_now_state == 1) { if ((r = read_tree_cost(c, c->scene.d_cost_now, c->scene.cost_now))) return r; c->scene.cost_now_state = 2; }
    out2[0] = c->scene.cost_now; out2[1] = c->scene.cost_base;
    return RTX_OK;
}

// rtx_scene_host.cpp — host-side scene assembly: material packing, the light list with its CDF, world-space flattening and shade records, and SceneHost::build, which
// lists the steps of a commit (tree: rtx_bvh_build.cpp / rtx_bvh_wide.cpp, tiny-scene records: rtx_small_scene.cpp, any-hit probe: rtx_bvh_replay.cpp).  No HIP calls in this file.
#include "rtx_scene_host.hpp"
#include "rtx_normalmap_host.hpp"
#include "rtx_specmap_host.hpp"
#include "rtx_emimap_host.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <system_error>
#include <thread>

namespace rtx {

// float -> binary16 (round to nearest even) -> float.  `-enable-16bit-types` makes HLSL `half` a true
// binary16 (DXRHelper.h:125), so half4(mat.Kd) etc. round (Sampler_v6.hlsl:71-83).
float half_round(float x) {
    uint32_t u = f2u(x), sign = u & 0x80000000u, a = u & 0x7FFFFFFFu;
    if (a >= 0x7F800000u) return x;
    if (a >= 0x477FF000u) return u2f(sign | 0x7F800000u);
    if (a < 0x33000001u) return u2f(sign);
    if (a < 0x38800000u) {
        float r = nearbyintf(u2f(a) * 16777216.0f);
        return u2f(sign | f2u(r * (1.0f / 16777216.0f)));
    }
    uint32_t rem = a & 0x1FFFu, base = a & ~0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (base & 0x2000u))) base += 0x2000u;
    return u2f(sign | base);
}

// General 4x4 inverse by cofactors in double, rounded to float once (XMMatrixInverse stand-in:
// Renderer.cpp:1735-1736, 2101-2118).
void mat4_inverse(const float* mf, float* out) {
    double m[16], inv[16];
    for (int i = 0; i < 16; i++) m[i] = (double)mf[i];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    double det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    double id = 1.0 / det;
    for (int i = 0; i < 16; i++) out[i] = (float)(inv[i] * id);
}

// objectToWorldNormal = transpose(inverse(upper 3x3, rest identity)): Renderer.cpp:2104-2116
void normal_matrix(const float* o2w, float* out) {
    float u[16], inv[16];
    memcpy(u, o2w, 64);
    u[3] = u[7] = u[11] = 0.0f; u[12] = u[13] = u[14] = 0.0f; u[15] = 1.0f;
    mat4_inverse(u, inv);
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) out[c * 4 + r] = inv[r * 4 + c];
}

static inline f3 vpos(const MeshHost& m, uint32_t vi) { const float* p = &m.verts[(size_t)vi * 7]; return mk3(p[0], p[1], p[2]); }
static inline f3 vnrm(const MeshHost& m, uint32_t vi) { const float* p = &m.verts[(size_t)vi * 7]; return mk3(p[3], p[4], p[5]); }
static inline void copy_instance(InstGPU& g, const InstHost& in) { memcpy(g.o2w, in.o2w, 64); memcpy(g.nrm, in.nrm, 64); memcpy(g.o2w_inv, in.o2w_inv, 64); memcpy(g.prev_o2w, in.prev_o2w, 64); }
// the three object-space corners of triangle t of a mesh (input of the GPU refit)
static inline void put_objtri(const MeshHost& m, uint32_t t, F4* dst) { for (int k = 0; k < 3; k++) { const f3 p = vpos(m, m.idx[t * 3 + k]); dst[k] = {p.x, p.y, p.z, 0.0f}; } }

bool SceneHost::set_materials(const void* mats, uint32_t count) {
    if (!mats && count) { err = "materials pointer is null"; return false; }
    mats128.assign((const float*)mats, (const float*)mats + (size_t)count * 32);
    mats_dirty = true;
    for (uint32_t s = 0; s < kMapSlotCount; s++) {           // the table is replaced: no material of the new one has a map (the energy table is no material's: it stays)
        if (any_bound((MapSlot)s)) tex_dirty = true;
        maps[s].clear();
    }
    return true;
}

bool SceneHost::add_mesh(const void* verts28, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const uint32_t* mids, uint32_t* out) {
    if (!verts28 || !idx || !mids) { err = "add_mesh: null array"; return false; }
    if (nidx % 3) { err = "add_mesh: index count is not a multiple of 3"; return false; }
    const float* v = (const float*)verts28;
    for (uint32_t i = 0; i < nidx; i++) if (idx[i] >= nverts) { err = "add_mesh: index out of range"; return false; }
    // Vertex.normal.w is the model's base offset inside the global materialIDs[] (ObjLoader.h:466; Hit_v6.hlsl:17)
    for (uint32_t i = 0; i < nverts; i++)
        if ((uint32_t)v[(size_t)i * 7 + 6] != (uint32_t)matids.size()) { err = "add_mesh: Vertex.normal.w != materialIDs base offset of this mesh"; return false; }
    MeshHost m;
    m.verts.assign(v, v + (size_t)nverts * 7);
    m.idx.assign(idx, idx + nidx);
    m.matid_base = (uint32_t)matids.size();
    matids.insert(matids.end(), mids, mids + nidx);
    if (out) *out = (uint32_t)meshes.size();
    meshes.push_back(std::move(m));
    topo_dirty = true;
    return true;
}

bool SceneHost::add_instance(uint32_t mesh, const float* o2w, uint32_t* out) {
    if (mesh >= meshes.size()) { err = "add_instance: unknown mesh"; return false; }
    InstHost in; in.mesh = mesh; memcpy(in.o2w, o2w, 64); normal_matrix(o2w, in.nrm); in.tri_base = 0;
    mat4_inverse(o2w, in.o2w_inv); memcpy(in.prev_o2w, o2w, 64);          // Renderer.cpp:2098-2102
    if (out) *out = (uint32_t)insts.size();
    insts.push_back(in);
    topo_dirty = true;
    return true;
}

bool SceneHost::set_instance_transform(uint32_t inst, const float* o2w) {
    if (inst >= insts.size()) { err = "set_instance_transform: unknown instance"; return false; }
    memcpy(insts[inst].prev_o2w, insts[inst].o2w, 64);                        // prevObjectToWorld = last frame's objectToWorld
    memcpy(insts[inst].o2w, o2w, 64); normal_matrix(o2w, insts[inst].nrm); mat4_inverse(o2w, insts[inst].o2w_inv);
    return true;
}

bool SceneHost::set_instance_visible(uint32_t inst, bool visible, bool* changed) {
    if (inst >= insts.size()) { err = "set_instance_visible: unknown instance"; return false; }
    *changed = is_hidden(inst) == visible;
    if (*changed) { if (inst_hidden.size() < insts.size()) inst_hidden.resize(insts.size(), 0); inst_hidden[inst] = visible ? 0 : 1; }
    return true;
}
void SceneHost::commit_visibility(BuiltScene& B) const {
    B.inst_hidden.assign(insts.size(), 0u); B.any_hidden = false;
    for (size_t ii = 0; ii < insts.size(); ii++) if (is_hidden(ii)) { B.inst_hidden[ii] = 1u; B.any_hidden = true; }
}

bool SceneHost::update_mesh_vertices(uint32_t mesh, const void* verts28, uint32_t nverts) {
    if (mesh >= meshes.size()) { err = "update_mesh_vertices: unknown mesh"; return false; }
    if (!verts28) { err = "update_mesh_vertices: null array"; return false; }
    MeshHost& m = meshes[mesh];
    if ((size_t)nverts * 7 != m.verts.size()) { err = "update_mesh_vertices: vertex count differs from the mesh's (topology changes need a new mesh)"; return false; }
    const float* v = (const float*)verts28;
    for (uint32_t i = 0; i < nverts; i++)
        if ((uint32_t)v[(size_t)i * 7 + 6] != m.matid_base) { err = "update_mesh_vertices: Vertex.normal.w != materialIDs base offset of this mesh"; return false; }
    m.verts.assign(v, v + (size_t)nverts * 7);
    if (!mesh_is_dirty(mesh)) dirty_meshes.push_back(mesh);
    return true;
}

bool SceneHost::set_mesh_uvs(uint32_t mesh, const float* uv2, uint32_t nidx) {
    if (mesh >= meshes.size()) { err = "set_mesh_uvs: unknown mesh"; return false; }
    MeshHost& m = meshes[mesh];
    if (!uv2) { if (!m.uvs.empty()) { m.uvs.clear(); tex_dirty = true; } return true; }
    if (nidx != m.idx.size()) { err = "set_mesh_uvs: one (u, v) pair per index entry of the mesh"; return false; }
    for (size_t i = 0; i < (size_t)nidx * 2; i++) if (!std::isfinite(uv2[i])) { err = "set_mesh_uvs: non-finite coordinate"; return false; }
    m.uvs.assign(uv2, uv2 + (size_t)nidx * 2);
    tex_dirty = true;
    return true;
}
bool SceneHost::set_texture(uint32_t tex, const void* rgba8, uint32_t width, uint32_t height, uint32_t flags) {
    if (tex > textures.size()) { err = "set_texture: texture id beyond the end of the table (the current count appends)"; return false; }
    if (!rgba8) { err = "set_texture: null pixel pointer"; return false; }
    if (width < 1 || width > 16384 || height < 1 || height > 16384) { err = "set_texture: width and height must be in [1, 16384]"; return false; }
    if (flags & ~1u) { err = "set_texture: unknown flag bits"; return false; }
    uint64_t total = (uint64_t)width * height;
    for (size_t i = 0; i < textures.size(); i++) if (i != tex) total += textures[i].rgba.size();
    if (total > 0x7FFFFFFFull) { err = "set_texture: more than 2^31 texels in the table"; return false; }
    if (tex == textures.size()) textures.emplace_back();
    TexHost& t = textures[tex];
    t.width = width; t.height = height; t.flags = flags;
    t.rgba.assign((const uint32_t*)rgba8, (const uint32_t*)rgba8 + (size_t)width * height);
    tex_dirty = true;
    return true;
}
bool SceneHost::set_material_map(uint32_t material, uint32_t slot, int32_t tex) {
    if (material >= mats128.size() / 32) { err = "set_material_map: unknown material"; return false; }
    const uint32_t s = map_slot_of(slot);
    if (s == kMapSlotCount) { err = "set_material_map: unknown slot (RTX_MAP_KD = 0, RTX_MAP_OPACITY = 2, RTX_MAP_NORMAL = 4, RTX_MAP_KS = 6, RTX_MAP_PR = 8, RTX_MAP_PM = 10 or RTX_MAP_KE = 12)"; return false; }
    if (tex < -1 || (tex >= 0 && (size_t)tex >= textures.size())) { err = "set_material_map: unknown texture"; return false; }
    std::vector<int32_t>& map = maps[s];
    if (map.size() < mats128.size() / 32) map.resize(mats128.size() / 32, -1);
    map[material] = tex;
    tex_dirty = true;
    return true;
}
bool SceneHost::set_ess_table(const float* table, uint32_t rows) {
    if (const char* e = ess_table_error(table, rows)) { err = e; return false; }
    if (rows) ess_table.assign(table, table + (size_t)rows * kEssCols); else ess_table.clear();
    ess_rows = rows;
    tex_dirty = true;
    return true;
}
MapUse SceneHost::map_use() const {
    // per material the groups a triangle of it activates, and their union: what a triangle can still add (most scenes bind nothing, and no triangle is looked at)
    std::vector<uint8_t> of_mat(mats128.size() / 32, 0);
    MapUse reachable, use;
    for (uint32_t s = 0; s < kMapSlotCount; s++)
        for (size_t mat = 0; mat < maps[s].size() && mat < of_mat.size(); mat++)
            if (bound_texture((MapSlot)s, (uint32_t)mat) >= 0) { of_mat[mat] |= (uint8_t)(1u << kMapSlots[s].group); reachable.groups |= of_mat[mat]; }
    for (size_t i = 0; i < matids.size() && use != reachable; i += 3)      // (a triangle's material is the id of its first index entry: flatten_range)
        if (matids[i] < of_mat.size()) use.groups |= of_mat[matids[i]];
    return use;
}
void SceneHost::fill_tri_cut(std::vector<int32_t>& out) const {
    size_t nt = 0; for (const InstHost& in : insts) nt += meshes[in.mesh].idx.size() / 3;
    out.assign(nt, -1);
    for (const InstHost& in : insts) {
        const MeshHost& m = meshes[in.mesh];
        for (size_t t = 0; t < m.idx.size() / 3; t++) out[(size_t)in.tri_base + t] = bound_texture(kMapOpacity, matids[m.matid_base + 3 * t]);
    }
}
void SceneHost::fill_tri_tan(std::vector<float>& out) const {
    size_t nt = 0; for (const InstHost& in : insts) nt += meshes[in.mesh].idx.size() / 3;
    out.assign(nt * 6, 0.0f);
    const float zero_uv[6] = {0, 0, 0, 0, 0, 0};
    for (const InstHost& in : insts) {
        const MeshHost& m = meshes[in.mesh];
        for (size_t t = 0; t < m.idx.size() / 3; t++) {
            float p[9];
            for (int k = 0; k < 3; k++) memcpy(p + 3 * k, &m.verts[(size_t)m.idx[t * 3 + k] * 7], 12);
            tangent_record(p, m.uvs.empty() ? zero_uv : &m.uvs[t * 6], &out[((size_t)in.tri_base + t) * 6]);
        }
    }
}
bool SceneHost::only_maps_changed(const BuiltScene& b) const {
    if (topo_dirty || mats_dirty || !dirty_meshes.empty() || b.insts.size() != insts.size()) return false;
    for (size_t ii = 0; ii < insts.size(); ii++) {
        if (memcmp(b.insts[ii].o2w, insts[ii].o2w, 64) != 0 || memcmp(b.insts[ii].prev_o2w, insts[ii].prev_o2w, 64) != 0) return false;
        if ((ii < b.inst_hidden.size() && b.inst_hidden[ii] != 0u) != is_hidden(ii)) return false;
    }
    return true;
}
void SceneHost::fill_tri_uv(std::vector<float>& out) const {
    size_t nt = 0; for (const InstHost& in : insts) nt += meshes[in.mesh].idx.size() / 3;
    out.assign(nt * 6, 0.0f);
    for (const InstHost& in : insts) {
        const MeshHost& m = meshes[in.mesh];
        if (!m.uvs.empty()) memcpy(&out[(size_t)in.tri_base * 6], m.uvs.data(), m.uvs.size() * 4);      // corner k of triangle t = index entry 3 t + k
    }
}

static bool mesh_emits(const SceneHost& H, const MeshHost& m) {
    const uint32_t nmat = (uint32_t)(H.mats128.size() / 32);
    for (size_t i = 0; i < m.idx.size(); i++) {
        const uint32_t id = H.matids[m.matid_base + i];
        if (id < nmat && H.mats128[(size_t)id * 32 + 8] + H.mats128[(size_t)id * 32 + 9] + H.mats128[(size_t)id * 32 + 10] > 0.0f) return true;
    }
    return false;
}
bool SceneHost::dirty_mesh_emits() const {
    for (uint32_t mesh : dirty_meshes) if (mesh_emits(*this, meshes[mesh])) return true;
    return false;
}
bool SceneHost::instance_emits(size_t inst) const { return mesh_emits(*this, meshes[insts[inst].mesh]); }

void SceneHost::build_lights(BuiltScene& B) const {
    const uint32_t nmat = (uint32_t)(mats128.size() / 32);
    // ---- emissive triangle list + CDF: Renderer.cpp:2123-2233, 2237-2243 ----
    // EMISSION MAPS (include/rtx.h): while one is active the weight of a mapped emitter triangle follows the mean of its texels (rtx_emimap_host.hpp), every light carries
    // its global triangle id and emission texture, and q per global triangle id is what the emissive hit's MIS pdf reads.  Inactive: the scan as it always was, nothing more
    const bool emi = map_use().emi();
    B.emi_q.clear(); B.light_emi.clear();
    if (emi) { size_t nt = 0; for (const InstHost& in : insts) nt += meshes[in.mesh].idx.size() / 3; B.emi_q.assign(nt, 0.0f); }
    const float zero_uv[6] = {0, 0, 0, 0, 0, 0};
    struct Tmp { float w, w_plain; uint32_t order; uint32_t inst; f3 p0, p1, p2; float em[3]; uint32_t prim; int32_t tex; };
    std::vector<Tmp> tmp;
    for (size_t ii = 0; ii < insts.size(); ii++) {
        if (is_hidden(ii)) continue;                                 // InstanceMask 0: its emitters are no lights (the list of the scene without the instance, instance ids kept)
        const MeshHost& m = meshes[insts[ii].mesh];
        for (uint32_t t = 0; t < m.idx.size() / 3; t++) {
            uint32_t m0 = matids[m.matid_base + t * 3], m1 = matids[m.matid_base + t * 3 + 1], m2 = matids[m.matid_base + t * 3 + 2];
            if (m0 >= nmat) continue;
            const float* mat = &mats128[(size_t)m0 * 32];
            float inten = (mat[8] + mat[9] + mat[10]) / 3.0f;
            const float inten_plain = inten;
            int32_t tex = -1;
            if (emi && (mat[8] + mat[9] + mat[10] > 0.0f)) {          // (a hit reads the material of the first index entry: q is filled before the scan's own filters)
                float E[3] = {mat[8], mat[9], mat[10]};
                tex = bound_texture(kMapKe, m0);
                if (tex >= 0) {
                    const TexHost& T = textures[tex];
                    float mean[3];
                    emi_triangle_mean(T.rgba.data(), T.width, T.height, (T.flags & 1u) != 0u, m.uvs.empty() ? zero_uv : &m.uvs[(size_t)t * 6], mean);
                    inten = emi_intensity(&mat[8], mean, E);
                }
                B.emi_q[(size_t)insts[ii].tri_base + t] = (half_round(E[0]) + half_round(E[1]) + half_round(E[2])) / 3.0f;
            }
            if (m0 != m1 || m0 != m2) continue;                      // :2153-2156
            if (!(mat[8] + mat[9] + mat[10] > 0.0f)) continue;       // :2162
            Tmp L;
            L.p0 = vpos(m, m.idx[t * 3]); L.p1 = vpos(m, m.idx[t * 3 + 1]); L.p2 = vpos(m, m.idx[t * 3 + 2]);
            float area = 0.5f * length(cross(L.p1 - L.p0, L.p2 - L.p0));   // ComputeTriangleWeight :2217-2233
            L.w = area * inten; L.w_plain = area * inten_plain; L.order = (uint32_t)tmp.size(); L.inst = (uint32_t)ii;
            L.prim = insts[ii].tri_base + t; L.tex = tex;
            L.em[0] = mat[8]; L.em[1] = mat[9]; L.em[2] = mat[10];
            tmp.push_back(L);
        }
    }
    // sorted descending by weight, the running CDF, the 80-byte records.  black: the list of an active emission map whose total weight is 0 gets wn = 0
    auto fill = [&](std::vector<float>& rec80, float& total_out, bool black_ok) {
        // :2187-2190 sorts descending by weight with std::sort (unstable); ties are broken here by collection order
        std::sort(tmp.begin(), tmp.end(), [](const Tmp& a, const Tmp& b) { return a.w > b.w || (a.w == b.w && a.order < b.order); });
        float total = 0.0f;
        for (auto& L : tmp) total += L.w;
        total_out = total;
        rec80.assign(tmp.size() * 20, 0.0f);
        float cum = 0.0f;
        const uint32_t nl = (uint32_t)tmp.size();
        for (size_t i = 0; i < tmp.size(); i++) {
            Tmp& L = tmp[i];
            float wn = (black_ok && !(total > 0.0f)) ? 0.0f : L.w / total; cum += wn;     // (emission maps, total == 0: every map black, no emitter has weight — the renderer then gets no light list)
            float cdf = (i + 1 == tmp.size()) ? 1.0f : cum;             // :2208-2210
            float* r = &rec80[i * 20];
            r[0] = L.p0.x; r[1] = L.p0.y; r[2] = L.p0.z; r[3] = cdf;
            r[4] = L.p1.x; r[5] = L.p1.y; r[6] = L.p1.z; memcpy(&r[7], &L.inst, 4);
            r[8] = L.p2.x; r[9] = L.p2.y; r[10] = L.p2.z; r[11] = wn;
            r[12] = L.em[0]; r[13] = L.em[1]; r[14] = L.em[2]; memcpy(&r[15], &nl, 4);
            r[16] = total;
        }
    };
    // rtx_render_v6_pass1 and rtx_render_restir ignore the emission maps: while one is active they keep the list of the unmapped scene (area x mean(Ke)), built first
    B.lights80_plain.clear(); B.total_weight_plain = 0.0f;
    if (emi) {
        for (Tmp& L : tmp) std::swap(L.w, L.w_plain);
        fill(B.lights80_plain, B.total_weight_plain, false);
        for (Tmp& L : tmp) std::swap(L.w, L.w_plain);
    }
    fill(B.lights80, B.total_weight, emi);
    if (emi) for (const Tmp& L : tmp) { B.light_emi.push_back(L.prim); B.light_emi.push_back((uint32_t)L.tex); }
    refresh_lights(B);
}
// one device record from its 80-byte record: the corners through the instance's matrix, the light normal, the clamped area pdf
static void light_record(const SceneHost& H, const float* r, LightGPU& G) {
    uint32_t inst; memcpy(&inst, &r[7], 4);
    const f3 p0 = mk3(r[0], r[1], r[2]), p1 = mk3(r[4], r[5], r[6]), p2 = mk3(r[8], r[9], r[10]);
    const float cdf = r[3], wn = r[11];
    const float* M = H.insts[inst].o2w;
    f3 xv = xform_point(M, p0), yv = xform_point(M, p1), zv = xform_point(M, p2);
    f3 cl = cross(yv - xv, zv - xv);
    f3 nrm = normalize(cl);
    float area_l = fabsf(length(cl) * 0.5f);
    G.xv[0] = xv.x; G.xv[1] = xv.y; G.xv[2] = xv.z; G.cdf = cdf;
    G.yv[0] = yv.x; G.yv[1] = yv.y; G.yv[2] = yv.z; G.pdf_l = maxf_(kEps, wn / maxf_(area_l, kEps));
    G.zv[0] = zv.x; G.zv[1] = zv.y; G.zv[2] = zv.z; G.prim = 0u;
    G.em[0] = r[12]; G.em[1] = r[13]; G.em[2] = r[14]; G.emi_tex = 0;
    G.nl[0] = nrm.x; G.nl[1] = nrm.y; G.nl[2] = nrm.z; G.pad2 = 0.0f;
}
// the world-space half of the light records (the sample-independent part of SampleLightNEE_GI, Sampler_v6.hlsl:540-545, 566-575) from the 80-byte records, which hold the
// object-space corners, the instance, the weight and the CDF: all a TRANSFORM-only commit has to redo (which triangles emit, their weights and their order do not depend on
// the instance matrices — scanning the 11 M material ids of the street scene for them again was 3 ms of every refit commit)
void SceneHost::refresh_lights(BuiltScene& B) const {
    B.lights.resize(B.lights80.size() / 20);
    const bool emi = !B.lights.empty() && B.light_emi.size() == B.lights.size() * 2;      // (emission maps active: the triangle id and the texture; else both words 0, as they always were)
    for (size_t i = 0; i < B.lights.size(); i++) {
        light_record(*this, &B.lights80[i * 20], B.lights[i]);
        if (emi) { B.lights[i].prim = B.light_emi[i * 2]; B.lights[i].emi_tex = (int32_t)B.light_emi[i * 2 + 1]; }
    }
    B.lights_plain.resize(B.lights80_plain.size() / 20);             // (emission maps active: the unmapped scene's list beside it, for the renderers that ignore the maps)
    for (size_t i = 0; i < B.lights_plain.size(); i++) light_record(*this, &B.lights80_plain[i * 20], B.lights_plain[i]);
}

// transform-only commit on the GPU-refit path: the kernels re-derive triangles and boxes; the host re-derives what is small
bool SceneHost::refresh_transforms(BuiltScene& B) {
    if (topo_dirty || B.insts.size() != insts.size()) { err = "refresh_transforms: topology changed"; return false; }
    const bool mats_changed = mats_dirty;
    if (mats_dirty) build_materials(B);          // rtx_set_materials since the last commit: new table (the light list below reads the new Ke)
    B.inst_moved.assign(insts.size(), 0u);
    B.inst_hidden.resize(insts.size(), 0u);
    bool emitter_flipped = false;
    for (size_t ii = 0; ii < insts.size(); ii++) {
        const InstHost& in = insts[ii];
        const bool flipped = (B.inst_hidden[ii] != 0u) != is_hidden(ii);      // a visibility flip re-derives the same triangles and nodes: the never-hit record on or off, the boxes without or with them
        B.inst_moved[ii] = (memcmp(B.insts[ii].o2w, in.o2w, 64) != 0 || mesh_is_dirty(in.mesh) || flipped) ? 1u : 0u;      // (new vertices dirty the same triangles and nodes a new matrix does)
        if (flipped && !emitter_flipped && instance_emits(ii)) emitter_flipped = true;
        copy_instance(B.insts[ii], in);
    }
    commit_visibility(B);
    // new materials can change WHICH triangles emit, new vertices of an emitting mesh their areas, hence weights and order, a hidden or shown emitter the list itself: full scan
    // ... and so do new UVs, texels or map ids while an emission map is active, or was at the last commit: the weights follow the texels
    if (mats_changed || dirty_mesh_emits() || emitter_flipped || (tex_dirty && (B.map_use.emi() || map_use().emi()))) build_lights(B); else refresh_lights(B);
    B.refit_count++;
    return true;
}

// materials: MaterialOptimized rounding (Common_v6.hlsl:62-74).  Shared by the full build and by a commit that only changed materials
// (rtx_set_materials after the scene is resident: the BVH stays, the material table and the light list are re-derived).
void SceneHost::build_materials(BuiltScene& B) {
    const uint32_t nmat = (uint32_t)(mats128.size() / 32);
    B.mats.resize(nmat);
    for (uint32_t i = 0; i < nmat; i++) {
        const float* m = &mats128[(size_t)i * 32];   // Kd[4] Ks[3] Ni Ke[3] pad Pr_Pm_Ps_Pc[4] LUT[16]
        MatGPU& g = B.mats[i];
        for (int k = 0; k < 3; k++) { g.Kd[k] = half_round(m[k]); g.Ks[k] = half_round(m[4 + k]); g.Ke[k] = half_round(m[8 + k]); }
        g.Pr = half_round(m[12]); g.Pm = half_round(m[13]);
        g.KeFull[0] = m[8]; g.KeFull[1] = m[9]; g.KeFull[2] = m[10]; g.KeFullLen = length(mk3(m[8], m[9], m[10]));
        g.Ke_len = length(mk3(g.Ke[0], g.Ke[1], g.Ke[2]));
        for (int k = 0; k < 3; k++) g.KdPi[k] = g.Kd[k] / kPI;
        g.pad = 0.0f;
        g.alpha = half_round(m[3]); g.Ni = m[7]; g.pad1 = g.pad2 = 0.0f;      // MaterialOptimized.Kd.w (fp16) and the full-precision Material.Ni (strategy-3 extension)
        memcpy(g.LUT, m + 16, 64);
    }
    mats_dirty = false;
}

// first step of a geometry-changing commit: every instance gets its range of global triangle ids (consecutive, in instance order) and its device record; returns the triangle count
static uint32_t number_triangle_ranges(SceneHost& H, BuiltScene& B) {
    uint32_t nt = 0;
    for (auto& in : H.insts) { in.tri_base = nt; nt += (uint32_t)(H.meshes[in.mesh].idx.size() / 3); }
    B.insts.resize(H.insts.size());
    for (size_t ii = 0; ii < H.insts.size(); ii++) copy_instance(B.insts[ii], H.insts[ii]);
    H.commit_visibility(B);                     // a geometry-changing commit keeps every instance's visibility
    return nt;
}

// RTX_OPT_GPU_BUILD: the tree is the device's business (csrc/rtx_build.hip); nothing of it, nor of the per-triangle records, is mirrored on the host
static void forget_tree(BuiltScene& B, uint32_t nt) {
    B.shade.clear(); B.shade.shrink_to_fit(); B.objtris.clear(); B.objtris.shrink_to_fit();
    B.bvh_pad = 2e-6f; B.nodes.clear(); B.nodes8.clear(); B.tri_slots8.clear(); B.tris8.clear(); B.tris.clear(); B.leaf_order.clear(); B.level_start8.clear();
    B.small_recs.clear(); B.small_tris.clear(); B.small_poly.clear(); B.small_slabs.clear(); B.small_excess.clear(); B.small_slab_mask = 0; B.small_nrec = 0; B.small_nocc = 0; B.built_tris = nt; B.refit_count = 0; B.any_order = 0;
}

bool SceneHost::prepare_device_build(BuiltScene& B) {
    BuildStopwatch sw("[build] ", 28);
    build_materials(B);
    const uint32_t nt = number_triangle_ranges(*this, B);
    sw.lap("materials + instances");
    build_lights(B);
    sw.lap("lights");
    forget_tree(B, nt);
    topo_dirty = false;
    return true;
}

// object-space triangles of the GPU refit, re-derived from the meshes (what build() fills; a loaded cache does not carry them)
void SceneHost::fill_objtris(BuiltScene& B) const {
    size_t nt = 0; for (const InstHost& in : insts) nt += meshes[in.mesh].idx.size() / 3;
    B.objtris.resize(nt * 3);
    for (const InstHost& in : insts) {
        const MeshHost& m = meshes[in.mesh];
        for (uint32_t t = 0; t < m.idx.size() / 3; t++) put_objtri(m, t, &B.objtris[((size_t)in.tri_base + t) * 3]);
    }
}

// world-space corners, object-space corners and shade records (Hit_v6.hlsl:12-61) of the triangles [t_lo, t_hi) of instance ii; scale: running maximum of the world coordinates
static void flatten_range(const SceneHost& H, size_t ii, uint32_t t_lo, uint32_t t_hi, BuiltScene& B, std::vector<float>& wtri, float& scale) {
    const InstHost& in = H.insts[ii]; const MeshHost& m = H.meshes[in.mesh];
    for (uint32_t t = t_lo; t < t_hi; t++) {
        uint32_t g = in.tri_base + t;
        uint32_t i0 = m.idx[t * 3], i1 = m.idx[t * 3 + 1], i2 = m.idx[t * 3 + 2];
        const uint32_t vi[3] = {i0, i1, i2};
        put_objtri(m, t, &B.objtris[(size_t)g * 3]);
        for (int k = 0; k < 3; k++) {
            f3 w = xform_point(in.o2w, vpos(m, vi[k]));
            wtri[(size_t)g * 9 + k * 3] = w.x; wtri[(size_t)g * 9 + k * 3 + 1] = w.y; wtri[(size_t)g * 9 + k * 3 + 2] = w.z;
            scale = std::max(scale, std::max(fabsf(w.x), std::max(fabsf(w.y), fabsf(w.z))));
        }
        TriShade& s = B.shade[g];
        uint32_t mi = m.matid_base + 3 * t;    // == 3*PrimitiveIndex() + uint(v0.normal.w), Hit_v6.hlsl:16-17
        s.mat = mi < H.matids.size() ? H.matids[mi] : kMissMat;
        s.inst = (uint32_t)ii;
        f3 p0 = vpos(m, i0);
        f3 cr = cross(vpos(m, i1) - p0, vpos(m, i2) - p0);      // :28-30
        s.area = fabsf(length(cr) * 0.5f);                      // :31
        f3 flat = normalize(cr);                                // :32
        s.flat[0] = flat.x; s.flat[1] = flat.y; s.flat[2] = flat.z;
        float* dst[3] = {s.n0, s.n1, s.n2};
        for (int k = 0; k < 3; k++) {                           // :40-46 (all(n != 0) is per component)
            f3 nk = vnrm(m, vi[k]);
            f3 use = (nk.x != 0.0f && nk.y != 0.0f && nk.z != 0.0f) ? nk : flat;
            dst[k][0] = use.x; dst[k][1] = use.y; dst[k][2] = use.z;
        }
        s.guard_tau = 0.0f;
    }
}

// ---- flatten instances to world-space triangles (9 floats each); per-triangle shade records and object-space triangles.  Returns the coordinate scale: the largest
//      absolute world coordinate, at least 1 ----
static float flatten_instances(const SceneHost& H, uint32_t nt, BuiltScene& B, std::vector<float>& wtri) {
    wtri.resize((size_t)nt * 9);
    B.shade.resize(nt);
    B.objtris.resize((size_t)nt * 3);
    float scale = 1.0f;
    for (size_t ii = 0; ii < H.insts.size(); ii++) {
        // (round 5) the triangles of a large mesh on up to 16 threads — every triangle writes its own records, the coordinate scale is a maximum: 0.26 s of the 3.8 M-triangle
        // street's commit on one core, and what is left of the host's work when the tree is built on the GPU
        const uint32_t ntm = (uint32_t)(H.meshes[H.insts[ii].mesh].idx.size() / 3);
        const unsigned hwc = std::thread::hardware_concurrency();
        const uint32_t nth = ntm >= 65536u ? std::min<uint32_t>(16u, std::max(1u, hwc ? hwc : 4u)) : 1u;
        std::vector<float> tscale(nth, 1.0f);
        if (nth <= 1) flatten_range(H, ii, 0, ntm, B, wtri, tscale[0]);
        else {
            std::vector<std::thread> pool;
            for (uint32_t k = 0; k < nth; k++) {
                const uint32_t lo_t = (uint32_t)((uint64_t)ntm * k / nth), hi_t = (uint32_t)((uint64_t)ntm * (k + 1) / nth);
                try { pool.emplace_back([&, lo_t, hi_t, k] { flatten_range(H, ii, lo_t, hi_t, B, wtri, tscale[k]); }); } catch (const std::system_error&) { flatten_range(H, ii, lo_t, hi_t, B, wtri, tscale[k]); }
            }
            for (std::thread& th : pool) th.join();
        }
        for (float v : tscale) scale = std::max(scale, v);
    }
    return scale;
}

// ---- BVH: full binned-SAH build, or a REFIT when only instance transforms changed since the last build
//      (the reference refits its TLAS every frame: Renderer.cpp:594, TopLevelASGenerator.cpp:149-250) ----
static void build_or_refit_bvh(SceneHost& H, BuiltScene& B, const std::vector<float>& wtri, uint32_t nt) {
    const bool refit = !H.topo_dirty && B.built_tris == nt && !B.leaf_order.empty() && !B.nodes.empty();
    if (refit) refit_bvh(wtri, B.bvh_pad, B.nodes, B.leaf_order);
    else { build_bvh(wtri, B.bvh_pad, B.nodes, B.leaf_order, B.max_depth, H.bvh); B.built_tris = nt; }
    B.refit_count = refit ? B.refit_count + 1 : 0;
    H.topo_dirty = false;
}

bool SceneHost::build(BuiltScene& B) {
    BuildStopwatch sw("[build] ", 28);
    build_materials(B);
    const uint32_t nt = number_triangle_ranges(*this, B);
    std::vector<float> wtri;
    const float scale = flatten_instances(*this, nt, B, wtri);
    sw.lap("flatten + shade records");
    build_lights(B);
    sw.lap("lights");
    B.bvh_pad = 2e-6f * scale;                  // absolute box padding (1e-5 measured 3 % slower; the relative margins kSlabLo / kSlabHi carry the triangle-test error)
    build_or_refit_bvh(*this, B, wtri, nt);
    sw.lap("build_bvh");
    leaf_triangles(wtri, B.leaf_order, B.tris);
    if (!wide_from_binary(B, bvh)) { err = "build: BVH collapse failed"; return false; }
    sw.lap("collapse_bvh8");
    // a tiny scene with a hidden instance takes the general BVH path until everything is visible again: its pre-test records, merged quads, hull faces and the NEE hull
    // shortcut are derived from geometry, and a hidden triangle may take part in none of them (identical results by the parity contract)
    // ... and so does one with an active texture map (k_bounce_small and k_primary_surface sample no image)
    // ... and one with an environment bound (k_bounce_small's misses end black)
    // ... and one with a cut-out triangle (the pre-test path runs no alpha test)
    // ... and one with an active normal map (k_bounce_small perturbs no normal)
    // ... and one with an active specular, roughness or metalness map (k_bounce_small reads the material table alone)
    // ... and one with an active emission map (k_bounce_small's emitters and light samples read no texel)
    B.map_use = map_use(); B.env_active = env.n != 0;
    if (B.any_hidden || B.map_use.any() || B.env_active) { B.small_recs.clear(); B.small_tris.clear(); B.small_poly.clear(); B.small_slabs.clear(); B.small_excess.clear(); B.small_slab_mask = 0; B.small_nrec = 0; B.small_nocc = 0; }
    else build_small_scene(B, wtri, scale);
    sw.lap("tris8 / small scene");
    B.any_order = probe_anyhit_order(B);
    sw.lap("probe");
    return true;
}

}  // namespace rtx

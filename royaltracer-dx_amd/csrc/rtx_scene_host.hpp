// rtx_scene_host.hpp — host-side scene state behind the C-ABI: what the reference's Renderer keeps in
// m_materials / m_materialIDs / m_VB / m_IB / m_instances / m_emissiveTriangles (Renderer.h:100-141),
// plus the BVH build that replaces the driver's BLAS/TLAS (Renderer.cpp:772-946; rtx_bvh_host.hpp).
#pragma once
#include <vector>
#include <string>
#include <stdint.h>
#include "rtx_types.hpp"
#include "rtx_bvh_host.hpp"
#include "rtx_env_host.hpp"
#include "rtx_map_slots.hpp"

namespace rtx {

float half_round(float x);                               // binary16 round trip (MaterialOptimized)
void  mat4_inverse(const float* m16, float* out16);      // XMMatrixInverse stand-in
void  normal_matrix(const float* o2w16, float* out16);   // Renderer.cpp:2104-2116

struct MeshHost { std::vector<float> verts; std::vector<uint32_t> idx; uint32_t matid_base = 0; std::vector<float> uvs; };      // uvs: (u, v) per INDEX entry (rtx_set_mesh_uvs), or empty = (0, 0) everywhere
struct TexHost { uint32_t width = 0, height = 0, flags = 0; std::vector<uint32_t> rgba; };      // rtx_set_texture: width x height RGBA8, row 0 on top
struct InstHost { uint32_t mesh; float o2w[16]; float nrm[16]; float o2w_inv[16]; float prev_o2w[16]; uint32_t tri_base; };

struct BuiltScene {
    std::vector<MatGPU>   mats;
    std::vector<NodeGPU>  nodes;      // binary tree (build / refit form, host only)
    std::vector<Node8GPU> nodes8;     // compressed 8-wide collapse of `nodes` (device traversal form)
    std::vector<uint32_t> tri_slots8; // leaf-order slot of each triangle in the wide tree's order
    std::vector<TriGPU>   tris8;      // `tris` permuted into that order (device copy)
    uint32_t stack8 = 0;              // traversal stack entries (sibling groups) the wide tree can need
    std::vector<uint32_t> level_start8; // breadth-first levels of nodes8: level l = [level_start8[l], level_start8[l+1]) (GPU refit sweeps them bottom-up)
    std::vector<F4>       objtris;    // object-space vertex positions, 3 per GLOBAL triangle id (input of the GPU refit)
    float bvh_pad = 0.0f;             // absolute padding of the leaf boxes used by the last host build
    std::vector<TriGPU>   tris;       // leaf order
    // tiny-scene path (only when the scene has <= kSmallSceneMaxTris triangles): pre-test records + their triangles
    std::vector<SmallRecPair> small_recs; std::vector<TriGPU> small_tris; uint32_t small_nrec = 0;
    std::vector<F4> small_poly;       // 4 corners per record (world space; a triangle repeats its last corner)
    std::vector<SmallSlabPair> small_slabs; uint32_t small_slab_mask = 0;   // slab form of the record pairs, one entry per SmallRecPair; bit kp set = pair kp is a slab pair (RTX_OPT_SMALL_SLABS)
    std::vector<float> small_excess;  // per record: excess area of its bounding parallelogram over the quad (fraction); -1 = not a quad
    uint32_t small_nocc = 0;          // records [0, small_nocc) can lie between two scene points; [small_nocc, small_nrec) are faces of the scene's convex hull
    float small_cm = 0.0f, small_delta = 0.0f;   // margin coefficient for t, distance tolerance of the edge planes
    float small_hull_margin = 0.0f;              // NEE origins must lie this far inside every hull-face plane to use the hull-face shortcut (TriShade::guard_tau)
    std::vector<TriShade> shade;      // global triangle id order
    std::vector<InstGPU>  insts;
    std::vector<LightGPU> lights;
    std::vector<float>    lights80;   // reference-layout LightTriangle records (20 floats each)
    std::vector<uint32_t> leaf_order;   // BVH leaf order (kept for refits): the triangle behind every leaf REFERENCE — a permutation unless spatial splits duplicated some
    uint32_t any_order = 0;             // visiting order of any-hit rays chosen by probe_anyhit_order (0 slot order, 1 nearest octant first, 2 farthest first)
    uint32_t built_tris = 0;            // triangle count the topology was built for
    float total_weight = 0.0f;
    uint32_t max_depth = 0;
    uint32_t refit_count = 0;           // commits since the last full build that only refitted the boxes
    std::vector<uint32_t> inst_hidden;  // one word per instance, non-zero = hidden, AS COMMITTED: what the resident tree's boxes, the never-hit triangle records and the light list reflect (the refit kernels read it)
    bool any_hidden = false;            // ... and whether any word of it is set
    MapUse map_use;                     // SceneHost::map_use() AS COMMITTED: while any() a tiny scene runs on the general path and DevScene::tri_uv / map_kd are set; per group, the DevScene members rtx_map_slots.hpp names
    bool env_active = false;            // an environment is bound (SceneHost::env.n != 0) AS COMMITTED: a tiny scene then runs on the general path
    // emission maps (include/rtx.h, EMISSION MAPS; rtx_emimap_host.hpp)
    std::vector<float> emi_q;           // build_lights while an emission map is active: q per GLOBAL triangle id (what the emissive hit's MIS pdf reads); else empty
    std::vector<uint32_t> light_emi;    // ... and per light of `lights`, in its order: global triangle id, emission texture id bits (0xFFFFFFFF = none); else empty
    std::vector<LightGPU> lights_plain; std::vector<float> lights80_plain; float total_weight_plain = 0.0f;      // ... and the list of the UNMAPPED scene, which rtx_render_v6_pass1 and rtx_render_restir keep sampling; else empty
    std::vector<uint32_t> inst_moved;   // refresh_transforms: 1 = the instance's objectToWorld differs from the last commit's, or its mesh's vertices do, or its visibility does (the GPU refit touches the triangles and nodes of these only)
};

struct SceneHost {
    std::vector<float> mats128;                 // count * 32 floats
    std::vector<MeshHost> meshes;
    std::vector<uint32_t> matids;               // global materialIDs[]
    std::vector<InstHost> insts;
    std::string err;
    bool topo_dirty = true;                     // meshes / instances added since the last build (a transform change alone refits)
    bool mats_dirty = true;                     // rtx_set_materials since the material table was last derived
    std::vector<uint32_t> dirty_meshes;         // rtx_update_mesh_vertices since the last commit: meshes whose vertices changed (topology kept; the commit clears the list)
    std::vector<uint8_t> inst_hidden;           // rtx_set_instance_visible: 1 = hidden, as the caller wants it from the next commit on; shorter than insts = the rest is visible (every instance starts visible)
    // diffuse texture maps (include/rtx.h: rtx_set_mesh_uvs, rtx_set_texture, rtx_set_material_map)
    std::vector<TexHost> textures;
    std::vector<int32_t> maps[kMapSlotCount];   // per slot (rtx_map_slots.hpp), per material: the texture id bound or -1; shorter than the table = the rest has none (rtx_set_materials empties them all)
    std::vector<float> ess_table; uint32_t ess_rows = 0;        // rtx_set_ess_table: rows x 16 floats, or empty / 0 (a table edit like the maps: tex_dirty; rtx_set_materials keeps it)
    bool tex_dirty = false;                     // one of the four setters (UVs, texture, material map, energy table) since the last commit
    // environment lighting (include/rtx.h: rtx_set_environment; rtx_env_host.hpp)
    EnvHost env;
    bool env_dirty = false;                     // rtx_set_environment since the last commit
    BvhBuildOptions bvh = bvh_build_options();  // builder knobs of this scene (rtx_set_option RTX_OPT_BVH_*)

    bool set_materials(const void* mats, uint32_t count);
    bool add_mesh(const void* verts28, uint32_t nverts, const uint32_t* idx, uint32_t nidx, const uint32_t* matids, uint32_t* out);
    bool add_instance(uint32_t mesh, const float* o2w, uint32_t* out);
    bool set_instance_transform(uint32_t inst, const float* o2w);
    // instanceDescs[i].InstanceMask (TopLevelASGenerator.cpp:198): all or nothing.  *changed = the value differs from the one held (false: nothing to commit)
    bool set_instance_visible(uint32_t inst, bool visible, bool* changed);
    bool is_hidden(size_t inst) const { return inst < inst_hidden.size() && inst_hidden[inst] != 0; }
    bool any_hidden() const { for (uint8_t h : inst_hidden) if (h) return true; return false; }
    void commit_visibility(BuiltScene& out) const;     // out.inst_hidden / any_hidden := the caller's values
    bool instance_emits(size_t inst) const;     // the instance's mesh carries a triangle that emits under the current material table
    // new positions and normals for a mesh whose topology stays (BottomLevelASGenerator.cpp:185-209, updateOnly): same vertex count, same Vertex.normal.w; on failure nothing changes
    bool update_mesh_vertices(uint32_t mesh, const void* verts28, uint32_t nverts);
    bool mesh_is_dirty(uint32_t mesh) const { for (uint32_t m : dirty_meshes) if (m == mesh) return true; return false; }
    bool dirty_mesh_emits() const;              // a dirty mesh carries a triangle that emits under the current material table (the light list then needs the full scan: weights and order depend on areas)
    // each returns false, with `err` set and NOTHING changed, for the RTX_ERR_INVALID cases of include/rtx.h
    bool set_mesh_uvs(uint32_t mesh, const float* uv2, uint32_t nidx);
    bool set_texture(uint32_t tex, const void* rgba8, uint32_t width, uint32_t height, uint32_t flags);
    bool set_material_map(uint32_t material, uint32_t slot, int32_t tex);
    bool any_bound(MapSlot slot) const { for (int32_t t : maps[slot]) if (t >= 0) return true; return false; }
    // the texture that slot `slot` gives a triangle whose material (the id of its first index entry) is `mat`, or -1: the material has the map AND the slot's rule (kMapSlots) lets it
    // act there — an emitter's opacity, normal and specular maps have no effect (opacity: what is left are the CUT-OUT TRIANGLES), an emission map acts on an emitter only
    int32_t bound_texture(MapSlot slot, uint32_t mat) const {
        if (mat >= maps[slot].size() || maps[slot][mat] < 0 || mat >= mats128.size() / 32) return -1;
        const MapRule rule = kMapSlots[slot].rule;
        return rule == kMapAnyMaterial || material_emits(mat) == (rule == kMapOnlyOnEmitter) ? maps[slot][mat] : -1;
    }
    MapUse map_use() const;                     // which groups are active: a material that some triangle uses has a map of the group whose rule lets it act (one pass over the triangles)
    bool set_ess_table(const float* table, uint32_t rows);
    bool material_emits(uint32_t mat) const { const float* m = &mats128[(size_t)mat * 32]; return m[8] > 0.0f || m[9] > 0.0f || m[10] > 0.0f; }      // a component of Ke is > 0
    void fill_tri_cut(std::vector<int32_t>& out) const;     // bound_texture(kMapOpacity, ..) per global triangle id (numbered like fill_tri_uv)
    void fill_tri_tan(std::vector<float>& out) const;       // the tangent record (rtx_normalmap_host.hpp) per global triangle id (numbered like fill_tri_uv), from the meshes' current object-space vertices
    bool only_maps_changed(const BuiltScene& b) const;      // against the committed scene b: no instance moved, was hidden or shown, no mesh got new vertices, same topology and material table
    void fill_tri_uv(std::vector<float>& out) const;        // 6 floats per global triangle id (InstHost::tri_base as the last geometry-changing commit numbered them)
    bool build(BuiltScene& out);                // the host's whole commit: materials, flattening + shade records, lights, the tree (built, or refitted after a transform-only change), its wide form, tiny-scene records, any-hit probe
    void build_materials(BuiltScene& out);      // mats128 -> MatGPU table (clears mats_dirty)
    // transform- or vertex-only update of the records the GPU refit does not derive itself: instance matrices and the light list; inst_moved also names the instances of dirty meshes
    bool refresh_transforms(BuiltScene& out);
    void build_lights(BuiltScene& out) const;
    void refresh_lights(BuiltScene& out) const; // the world-space half of the light records from lights80 (transform-only commits)
    // RTX_OPT_GPU_BUILD: everything of a geometry-changing commit EXCEPT the per-triangle work (flatten, shade records, tree), which the device does from the meshes themselves
    // (csrc/rtx_build.hip: k_flatten): materials, instance records and triangle ranges, lights.  out.shade / objtris / trees are left empty, out.built_tris = the triangle count
    bool prepare_device_build(BuiltScene& out);
    void fill_objtris(BuiltScene& out) const;   // object-space triangles for the GPU refit (not stored in a cache file)
};

// binary scene cache (rtx_scene_cache.cpp): the host scene + everything build() derived that the device needs; versioned, checksummed
// cam12 (optional): eye, center, up, fovY degrees, znear, zfar of the host layer's scene (rtxh_scene_save / rtxh_scene_load)
// aux (optional): data the host layer keeps beside the scene and this layer only carries — fixed-size records (MaterialExt, index-aligned with the material
// table) and a text blob (the texture file names, each NUL-terminated); both empty for a context-level save
struct CacheAux { uint32_t rec_bytes = 0; std::vector<uint8_t> records; std::vector<char> text; };
bool save_scene_cache(const SceneHost& H, const BuiltScene& B, const char* path, std::string& err, const float* cam12 = nullptr, const CacheAux* aux = nullptr);
bool load_scene_cache(const char* path, SceneHost& H, BuiltScene& B, std::string& err, float* cam12 = nullptr, CacheAux* aux = nullptr);

// the tiny-scene pre-test records (rtx_small_scene.cpp): from B.leaf_order / B.tris / B.shade / B.mats / B.insts, the world-space triangles (9 floats each) and the coordinate
// scale to B.small_* and TriShade::guard_tau; leaves them empty for a scene of more than kSmallSceneMaxTris triangles
void build_small_scene(BuiltScene& B, const std::vector<float>& wtri, float scale);

}  // namespace rtx

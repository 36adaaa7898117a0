// Scenes.h — host-side scene container + the synthetic scenes BASELINE.json names.  None of Cornell / Sponza /
// Bistro ship with the reference (only garage.obj / monke.obj do, Renderer.cpp:363), so they are generated here,
// deterministically, in the reference's own data model: a global Material table, per-model Vertex / index /
// materialID arrays (ObjLoader.h:393-495) and an instance list of (model, matrix) pairs (Renderer.h:106).
#pragma once
#include <string>
#include <vector>
#include "Vertex.h"
#include "ObjLoader.h"
#include "../../include/rtx.h"
#include "../csrc/rtx_map_slots.hpp"

struct SceneModel { std::vector<Vertex> vertices; std::vector<UINT> indices; std::vector<UINT> materialIDs;
                    std::vector<float> uvs; };      // one (u, v) per entry of `indices` (the OBJ's vt, per corner), or empty
struct SceneImage { uint32_t width = 0, height = 0; std::vector<uint8_t> rgba; uint32_t channels = 0; };      // a decoded texture, top-down RGBA8; width 0 = not loaded; channels: the file's own (1, 3 or 4)
struct SceneInstance { UINT model; XMMATRIX transform; };
// an environment map for rtx_set_environment: n x n octahedral float RGB (n = 0: none), the 16-float env_to_world (haveRotation false: identity), scale, RTX_ENV_* flags
struct SceneEnvironment { uint32_t n = 0; std::vector<float> rgb; bool haveRotation = false; float toWorld[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}; float scale = 1.0f; uint32_t flags = 0; };
// the two ways the command line makes one: a constant sky, and a latitude-longitude image file (Radiance .hdr / colour .pfm: host/ImageIO.h) resampled to n x n and turned by
// yaw degrees about +Y; the second throws std::runtime_error for a file that cannot be read
SceneEnvironment MakeSkyEnvironment(float r, float g, float b);
SceneEnvironment LoadEnvironment(const std::string& file, uint32_t n, float yaw_deg, float scale, bool hidden);
struct Scene {
    std::string name;
    std::vector<Material> materials;         // [default_0, mats of model 0..., default_1, ...]  (ObjLoader.h:415-417,494)
    std::vector<MaterialExt> materialExt;    // index-aligned with `materials` when the scene came from OBJ / MTL files (empty otherwise): the MTL fields and
    std::vector<std::string> textures;       // texture map ids the 128-byte record has no room for (Vertex.h:21 "ADD MAP IDs LATER"), and the distinct map file names
    std::vector<SceneImage> images;          // index-aligned with `textures`: the decoded map_Kd files (host/ImageIO readers); an entry that no map_Kd names, or whose file
                                             // is missing or in another format, stays empty.  BindSceneMaps hands the loaded ones to a context, sRGB-encoded
    std::vector<int> boundMaps[rtx::kMapSlotCount];   // per slot (csrc/rtx_map_slots.hpp), per material: the entry of `textures` BindSceneMaps binds there, or -1; empty = none.
                                             // LoadObjScene fills them: kMapKd the map_Kd; kMapOpacity the map_d, or with kCutoutsKdAlpha the 32-bit map_Kd (the alpha byte of such an image is the
                                             // file's own alpha channel (32-bit TGA) or its first channel (PGM / PPM / 24-bit TGA)); kMapNormal the norm image, or on request the map_Bump / bump
                                             // image, taken as a normal map or converted from a height map on load; kMapKs / kMapPr / kMapPm the map_Ks / map_Pr / map_Pm image (one packed file
                                             // may serve several slots); kMapKe the map_Ke image
    int boundMap(rtx::MapSlot slot, size_t material) const { return material < boundMaps[slot].size() ? boundMaps[slot][material] : -1; }
    std::vector<SceneModel> models;
    std::vector<SceneInstance> instances;
    XMFLOAT3 eye{0, 0, 1}, center{0, 0, 0}, up{0, 1, 0};
    float fovY_deg = 60.0f, zn = 0.1f, zf = 1000.0f;     // Renderer.cpp:1730-1731
    SceneEnvironment environment;            // bound by UploadScene, the Renderer and the N-GPU frame (every rank binds the same map); n = 0: the scene has none
    size_t triangles() const { size_t n = 0; for (auto& i : instances) n += models[i.model].indices.size() / 3; return n; }
};

Scene MakeCornellBox();                                             // 32 triangles, 2 emissive
// hard = false: uniformly tessellated stand-ins (every surface a grid of centimetre quads: the EASY case for a BVH builder); hard = true: the same shell, materials, light,
// camera and triangle budget with the size distribution of the real assets — a few triangles metres long beside ornament tessellated to millimetres, long thin trims,
// overlapping cloth, foliage (size ratio > 1000 : 1) — the case tree quality is FOR (Scenes.cpp: sponza_hard_build)
Scene MakeSponzaClass(uint32_t target_tris = 262144, uint32_t seed = 260, bool hard = false);
Scene MakeBistroClass(uint32_t target_tris = 3800000, uint32_t seed = 3800, bool hard = false);
// the reference's own startup scene: each file through ObjLoader::loadObjFile, one instance per model,
// instance 1 rotated 1.57 rad about Y (Renderer.cpp:363-407, 444-449)
// load_textures: decode every file a map_Kd names, relative to mtl_dir (a file that cannot be read is skipped with one line on stderr)
// cutouts (ignored without load_textures): kCutoutsOff = no opacity maps (the scene as it was before cut-outs existed); kCutoutsMapD = the images the map_d statements name —
// a map_d that names its material's map_Kd file is ONE texture in both slots; kCutoutsKdAlpha = additionally a material WITHOUT a map_d whose map_Kd file has an alpha channel of its
// own (32-bit TGA) gets that texture as its opacity map (opt-in: no existing scene changes)
enum SceneCutouts { kCutoutsOff = 0, kCutoutsMapD = 1, kCutoutsKdAlpha = 2 };
// normals (ignored without load_textures): which images become tangent-space normal maps (include/rtx.h, NORMAL MAPS).  kNormalsOff = none (the scene as it was before normal maps
// existed); kNormalsNorm = the images the `norm` statements name; kNormalsBumpAsNormal / kNormalsBumpHeight = additionally, for a material WITHOUT a norm, its map_Bump / bump image —
// taken as a normal map, or its channel 0 as a height map converted on load with HeightToNormalMap(strength) (csrc/rtx_normalmap_host.hpp).  flipY: DirectX-style maps (green =
// -bitangent): every normal map's green byte is negated on load (FlipGreen).  An image that another slot reads too is left as it is: the normal map is a copy appended to `textures`
enum SceneNormalMode { kNormalsOff = 0, kNormalsNorm = 1, kNormalsBumpAsNormal = 2, kNormalsBumpHeight = 3 };
struct SceneNormals { SceneNormalMode mode = kNormalsNorm; float strength = 1.0f; bool flipY = false; };
// spec_maps (ignored without load_textures): bind the images the map_Ks / map_Pr / map_Pm statements name (include/rtx.h, SPECULAR MAPS).  A map MULTIPLIES its material's scalar and
// the parser records a scalar the file does not give as 0, which would switch the map off: so binding a decoded map_Pr sets Pr == 0 to 1 (and regenerates the material's LUT),
// map_Pm likewise Pm, map_Ks a Ks of (0, 0, 0) to (1, 1, 1) (csrc/rtx_specmap_host.hpp) — a stated deviation from the reference's record, made only where a map is bound.
// false = none bound, the records as parsed
// emission_maps (ignored without load_textures): bind the image a map_Ke statement names (include/rtx.h, EMISSION MAPS); binding a decoded one sets a Ke of (0, 0, 0) to (1, 1, 1)
// (csrc/rtx_emimap_host.hpp), the same stated deviation, made only where a map is bound.  false = none bound, the records as parsed
Scene LoadObjScene(const std::vector<std::string>& files, const std::string& mtl_dir, bool load_textures = true, SceneCutouts cutouts = kCutoutsMapD, SceneNormals normals = SceneNormals(), bool spec_maps = true, bool emission_maps = true);
// rtx_set_mesh_uvs / rtx_set_texture / rtx_set_material_map (every slot a kernel samples) for what the scene carries, and — where a roughness map was bound — rtx_set_ess_table with
// 17 rows of GenerateEssLUT.  It only ADDS: slots and an energy table that an earlier scene left on the same context are not cleared (rtx_set_materials resets the slots; a
// table without a roughness map is read by nothing; rtx_set_ess_table(ctx, NULL, 0) clears it); a scene without a decoded image binds nothing.  Before rtx_commit_scene
int BindSceneMaps(const Scene&, rtx_ctx*);
// rtx_set_environment for what the scene carries (n = 0: clears the context's).  Before rtx_commit_scene
int BindSceneEnvironment(const SceneEnvironment&, rtx_ctx*);
// new vertices for a model whose topology stays (the scene-level twin of rtx_update_mesh_vertices, same checks: the model exists, same vertex count, Vertex.normal.w — the
// model's base in materialIDs[] — unchanged, non-null); false + err leaves the scene as it was
bool SetSceneMeshVertices(Scene&, UINT model, const void* verts28, uint32_t nverts, std::string& err);
// rtx_set_materials / rtx_add_mesh / rtx_add_instance / rtx_commit_scene / rtx_set_camera for `aspect`
int UploadScene(const Scene&, rtx_ctx*, float aspect);
void SceneViewProj(const Scene&, float aspect, float view[16], float proj[16]);

// Renderer.h — headless counterpart of the reference's Renderer class (Pathtracer/rdn/Renderer.h:46-51):
// same construction and OnInit / OnUpdate / OnRender / OnDestroy life cycle, no window, no DX12.  Everything
// the reference's Renderer feeds its shaders goes through the C-ABI of include/rtx.h instead.
#pragma once
#include <string>
#include <vector>
#include "Scenes.h"
#include "manipulator.h"

class Renderer {
public:
    Renderer(UINT width, UINT height, std::string name);
    ~Renderer();
    // headless configuration (the reference hard-codes these: Renderer.cpp:363, 46-48; Common_v6.hlsl:8-12)
    void SetModels(const std::vector<std::string>& obj_files, const std::string& mtl_dir) { m_models = obj_files; m_mtlDir = mtl_dir; m_haveScene = false; }
    void SetScene(const Scene& s) { m_scene = s; m_haveScene = true; }
    void SetCutouts(SceneCutouts c) { m_cutouts = c; }          // which opacity maps SetModels' OBJ files load (rtx_render --no-cutouts / --kd-alpha); the default is their map_d images
    void SetNormalMaps(SceneNormalMode mode, float strength = 1.0f, bool flipY = false) { m_normals.mode = mode; m_normals.strength = strength; m_normals.flipY = flipY; }      // which normal maps SetModels' OBJ files load (rtx_render --no-normal-maps / --bump-as-normal / --bump-height / --normal-flip-y); the default is their norm images
    void SetSpecMaps(bool on) { m_specMaps = on; }              // false: SetModels' OBJ files bind no map_Ks / map_Pr / map_Pm image (rtx_render --no-spec-maps)
    void SetEmissionMaps(bool on) { m_emissionMaps = on; }      // false: SetModels' OBJ files bind no map_Ke image (rtx_render --no-emission-maps)
    void SetLoadTextures(bool on) { m_loadTextures = on; }      // false: SetModels' OBJ files load without their map_Kd images (rtx_render --no-textures)
    void SetDevice(int ordinal) { m_device = ordinal; }
    rtx_params& Params() { return m_params; }
    // What OnRender issues.  ReSTIR = the reference's shipping frame, its three DispatchRays (Renderer.cpp:646-673: RayGen = pass 1, RayGen2 = temporal reuse,
    // RayGen3 = spatial reuse + shade) with its shader defines nee_samples 4 / bounces 3 (Common_v6.hlsl:8-12) unless RestirParams() is changed; one frame per
    // OnRender, history carried in the context.  PathTracer (the default of this headless build) = Params().spp samples of the bounce-loop estimator.
    enum class Mode { PathTracer, ReSTIR };
    void SetMode(Mode m) { m_mode = m; }
    Mode GetMode() const { return m_mode; }
    rtx_params& RestirParams() { return m_restir; }
    // m_instances[i].second = ... of the reference's OnUpdate (Renderer.cpp:444-449): the matrix takes effect in the next OnUpdate, which hands it to the context and
    // re-commits — a transform-only commit, i.e. a REFIT of the resident tree on the GPU (the reference refits its TLAS every frame, Renderer.cpp:594, 2091-2121)
    void SetInstanceTransform(UINT instance, const XMMATRIX& objectToWorld);
    // new vertices for a model whose topology stays (a skinned character, a cloth): taken now, handed to the context in the next OnUpdate (rtx_update_mesh_vertices), whose
    // commit refits the resident tree — the reference's helper has the door (BottomLevelASGenerator.cpp:185-209, updateOnly), its Renderer never opens it.  Throws
    // std::invalid_argument for an unknown model, another vertex count or a changed Vertex.normal.w
    void SetMeshVertices(UINT mesh, const std::vector<Vertex>& vertices);
    // instanceDescs[i].InstanceMask (TopLevelASGenerator.cpp:198) as all or nothing: the instance exists for no ray from the next OnUpdate on (rtx_set_instance_visible), whose
    // commit refits the resident tree; ids stay.  The value the instance already has changes nothing.  Throws std::out_of_range for an unknown instance
    void SetInstanceVisible(UINT instance, bool visible);
    // environment lighting (rtx_set_environment): before OnInit it is bound with the scene; afterwards the next OnUpdate hands it to the context and re-commits (tables only).
    // An environment with n = 0 clears it
    void SetEnvironment(const SceneEnvironment& env);
    // the thin-lens camera (rtx_set_lens): aperture radius and focus distance in world units, radius 0 = the pinhole.  Camera state: before OnInit it is kept and set with the
    // context, afterwards it takes effect at once — no commit, and like a camera move it leaves the accumulation to the caller
    void SetLens(float radius, float focus);
    // autofocus (rtx_focus_distance_at): the view-axis depth of what pixel (x, y) of the window sees first through the current camera, 0 = nothing.  After OnInit
    float FocusDistanceAt(UINT x, UINT y);
    double LastRefitMs() const { return m_refitMs; }

    void OnInit();      // Renderer.cpp:44-103: camera lookat, load models, build acceleration structures, upload
    void OnUpdate();    // Renderer.cpp:431-452: camera buffer, instance 1 rotation, instance properties
    void OnRender();    // Renderer.cpp:468-506 / 556-715: one frame = Params().spp samples per pixel, accumulated
    void OnDestroy();   // Renderer.cpp:546-552

    UINT GetWidth() const { return m_width; }
    UINT GetHeight() const { return m_height; }
    const std::string& GetTitle() const { return m_title; }
    uint32_t FrameIndex() const { return m_time; }
    std::vector<float> ReadAccumulation();          // gPermanentData (RGBA32F)
    // rtx_denoise over the accumulated image as it stands (nullptr = every default): the edge-avoiding a-trous filter guided by first-hit position, normal and material.
    // Path tracer frames only (std::logic_error in ReSTIR mode: that frame has its own reuse passes).  gPermanentData is left alone, so OnRender keeps accumulating; the
    // denoised image is read with ReadDenoised (RGBA32F, w = 1) / ReadDenoisedOutput (RGBA8 after the sRGB OETF).  Defined in RendererDenoise.cpp
    rtx_denoise_result Denoise(const rtx_denoise_params* params = nullptr);
    // rtx_denoise_variance: the same filter with the colour stop scaled by each pixel's own noise.  The image must have been sampled by rtx_render_adaptive on Context()
    // alone since its last clear (OnRender issues rtx_render: std::runtime_error after it, with the context's message); read like Denoise's.  Defined in RendererDenoise.cpp
    rtx_denoise_result DenoiseVariance(const rtx_denoise_var_params* params = nullptr);
    std::vector<float> ReadDenoised();
    std::vector<uint8_t> ReadDenoisedOutput();
    std::vector<uint8_t> ReadOutput();              // the DISPLAYED layer of gOutput (RGBA8): what the reference copies to the back buffer (Renderer.cpp:690-698)
    void OnKeyUp(uint8_t key);                      // 'C' cycles m_displayLevels (Renderer.cpp:748-754); other keys do nothing here (VK_SPACE toggles a raster path that does not exist)
    UINT CurrentDisplayLayer() const { return m_displayLevels[m_currentDisplayLevel]; }
    rtx_stats Stats();
    rtx_ctx* Context() { return m_ctx; }
private:
    void UpdateCameraBuffer();                      // Renderer.cpp:1722-1768
    void Check(int rc, const char* what);
    UINT m_width, m_height; float m_aspectRatio; std::string m_title;
    std::vector<std::string> m_models; std::string m_mtlDir;
    Scene m_scene; bool m_haveScene = false, m_loadTextures = true; SceneCutouts m_cutouts = kCutoutsMapD; SceneNormals m_normals; bool m_specMaps = true, m_emissionMaps = true;
    int m_device = 0;
    rtx_ctx* m_ctx = nullptr;
    rtx_params m_params{}, m_restir{};
    Mode m_mode = Mode::PathTracer;
    uint32_t m_time = 0;                             // Renderer.h: m_time
    UINT m_currentDisplayLevel = 0;                  // Renderer.h:298
    std::vector<UINT> m_displayLevels = {0, 10, 11, 12, 13, 14, 15, 16, 17, 20, 21, 22, 23, 24, 25, 26, 27, 28};   // Renderer.h:299
    float m_prevView[16]; bool m_havePrev = false;   // m_prevViewMatrix
    std::vector<UINT> m_movedInstances, m_changedMeshes; double m_refitMs = 0.0;
    SceneEnvironment m_env; bool m_haveEnv = false, m_envDirty = false;       // SetEnvironment: what it set (replaces the scene's own), and whether the context has yet to see it
    rtx_lens m_lens{};                                                        // SetLens: what it set (all zero = the pinhole)
    std::vector<uint8_t> m_hidden; std::vector<UINT> m_flippedInstances;      // visibility per instance as last asked for; the instances whose value changed since the last OnUpdate
};

// the handle of include/rtx_host.h's renderer functions (rtx_host_c.cpp; RendererDenoise.cpp for the one that needs the denoiser's entry points)
struct rtxh_renderer { Renderer* r; };

// rtx_render — headless CLI over the Renderer facade (replaces the Win32 window loop, Main.cpp:18-27).
// usage: rtx_render [--scene cornell|sponza|bistro|obj] [--obj a.obj,b.obj --mtl dir] [--w 1920 --h 1080]
//                   [--spp 64] [--frames 1] [--bounces 8] [--nee 1] [--lambert] [--out image.{png,ppm,exr}] [--device 0]
//                   [--mode pt|restir]   restir = the reference's shipping frame (3 DispatchRays, Renderer.cpp:646-673: pass 1 + temporal + spatial reuse), one per --frames,
//                   nee 4 / bounces 3 as in Common_v6.hlsl:8-12 unless --nee / --bounces are given; with --gpus N the shards own one tile rectangle each (RTX_FLAG_BLOCK_TILES,
//                   32-px tiles) and exchange history + framebuffer tiles once per frame; [--literal] = the thread-per-pixel kernels instead of the wavefront stages;
//                   [--halo px] with --gpus N --mode restir: the history travels as border strips of `px` pixels between neighbouring rectangles (one send + receive per
//                   neighbour, rtx_restir_pack_halo) instead of the all-gather of 140 B per pixel; the frame line then reports the bytes the busiest rank sent and the stale reads (must be 0);
//                   [--force-gather] with --gpus 1: pack -> RCCL all-gather of a one-rank communicator -> unpack all the same (exercises the collective path on one GPU);
//                   [--orbit deg] moves the camera about the look-at point between frames (exercises the reprojection)
//                   [--spin deg] turns instance 1 (the reference's moving instance, Renderer.cpp:444-449) by `deg` about the vertical axis before every frame after the first: a
//                   transform-only commit = a refit of the resident tree on the GPU, on every rank with --gpus N (the reference refits its TLAS every frame, Renderer.cpp:594)
//                   [--hide i[,j...]] hides the listed instances before the first frame (rtx_set_instance_visible: InstanceMask 0, TopLevelASGenerator.cpp:198)
//                   [--blink i] toggles the visibility of instance i before every frame after the first and prints the commit's time: a refit, never a rebuild
//                   [--only-rank r] with --gpus N --gather copy: rank r of N alone, through the same host path (measurement on one GPU: tools/shard_time.py native=1)
//                   [--adaptive THRESHOLD [--min-spp N] [--step-spp N]]   rtx_render_adaptive instead of rtx_render (path tracer, one GPU): every 256-slot chunk is sampled until its
//                   pixels pass the noise threshold, --spp is the cap (defaults: min 8, step 8; both even); prints the result struct per frame
//                   [--denoise [--denoise-levels N] [--sigma-color X] [--sigma-plane X]]   after the last frame rtx_denoise filters the accumulated image (edge-avoiding a-trous,
//                   guided by first-hit position, normal and material; defaults: 5 levels, 0.5, 2^-6 of the scene's extent) and --out gets the DENOISED image; works with
//                   --adaptive and with --gpus N (on rank 0, after the gather); refused with --mode restir (that frame has its own reuse passes)
//                   [--denoise-albedo] with --denoise: RTX_DENOISE_ALBEDO, the filter works on the image divided by the first hit's Kd' (texture detail survives)
//                   [--denoise-mapped-normals] with --denoise: RTX_DENOISE_MAPPED_NORMALS, the normal stop compares normal-mapped shading normals (shading relief survives);
//                   either one without --denoise is a usage error
//                   [--denoise-variance [--sigma-var K]] with --adaptive T: rtx_denoise_variance instead of rtx_denoise — the colour stop is scaled by each pixel's own noise, K
//                   standard deviations (default 4), estimated from the adaptive sampler's two half sums; implies --denoise, combines with --denoise-albedo and
//                   --denoise-mapped-normals, ignores --sigma-color; --adaptive 0 gives it a fixed --spp.  Without --adaptive, or with --gpus N > 1, a usage error
//                   [--no-textures]   OBJ scenes: do not read the images their map_Kd statements name (binary PPM / PGM, 24- / 32-bit TGA): the image without diffuse maps
//                   [--no-cutouts]    OBJ scenes: do not bind the images their map_d statements name as opacity maps (alpha cut-outs): the image with every card opaque
//                   [--kd-alpha]      OBJ scenes: a material without a map_d whose map_Kd is a 32-bit TGA gets that texture's alpha as its opacity map too
//                   [--no-normal-maps] OBJ scenes: do not bind the images their norm statements name as tangent-space normal maps: the image with flat-shaded walls
//                   [--bump-as-normal] a material without a norm takes its map_Bump / bump image as a normal map   [--bump-height S] ... as a height map (channel 0), converted on load with strength S
//                   [--normal-flip-y] DirectX-style normal maps (green = -bitangent): negate the green byte on load
//                   [--no-spec-maps]  OBJ scenes: do not bind the images their map_Ks / map_Pr / map_Pm statements name: one Ks, Pr and Pm per material, the records as parsed
//                   [--no-emission-maps] OBJ scenes: do not bind the image a map_Ke statement names: one Ke per material, the records as parsed
//                   [--env FILE [--env-res N] [--env-yaw DEG] [--env-scale S] [--env-hidden]]   environment lighting (rtx_set_environment): FILE is a latitude-longitude Radiance .hdr or
//                   colour .pfm, resampled to an N x N octahedral map (default 512), turned by DEG degrees about +Y, radiance times S; --env-hidden: camera rays that miss stay black
//                   [--sky R,G,B]   a constant sky of that radiance instead of a file; both work with --gpus N (every rank binds the same map) and are ignored by --mode restir
//                   [--aperture R [--focus D | --focus-pixel X,Y]]   the thin-lens camera (rtx_set_lens): aperture radius and focus distance in world units; --focus-pixel
//                   focuses on what that pixel sees before the first frame (rtx_focus_distance_at) and prints the distance, an explicit --focus wins; path tracer only
//                   (--mode restir keeps its pinhole); works with --gpus N (every rank gets the lens), --adaptive and --denoise
//                   [--gpus N [--devices 0,1,..] [--gather rccl|copy]]   the native N-GPU frame (MultiGpu.h): one process, N contexts, pixel tiles
//                   round-robin, ONE RCCL all-gather per frame; `--gather copy` replaces the collective by device copies (several ranks on one GPU: tests)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <fstream>
#include <functional>
#include <sstream>
#include <stdexcept>
#include <string>
#include "Renderer.h"
#include "ImageIO.h"
#include "MultiGpu.h"

static const char* kUsage =
    "usage: rtx_render [--scene cornell|sponza|bistro|obj] [--obj a.obj,b.obj --mtl dir] [--w 1920 --h 1080]\n"
    "                  [--spp 64] [--frames 1] [--bounces 8] [--nee 1] [--lambert] [--out image.{png,ppm,exr}] [--device 0]\n"
    "                  [--mode pt|restir] [--literal] [--halo px] [--force-gather] [--orbit deg] [--spin deg] [--hide i[,j...]] [--blink i] [--only-rank r]\n"
    "                  [--adaptive THRESHOLD [--min-spp N] [--step-spp N]]\n"
    "                  [--denoise [--denoise-levels N] [--sigma-color X] [--sigma-plane X]]   write the denoised image to --out (path tracer only)\n"
    "                  [--denoise-albedo] [--denoise-mapped-normals]   with --denoise: keep texture detail (filter the image divided by Kd') / normal-map relief\n"
    "                  [--denoise-variance [--sigma-var K]]   with --adaptive: scale the colour stop by each pixel's own noise (implies --denoise; one GPU)\n"
    "                  [--no-textures]   OBJ scenes: ignore map_Kd images (implies --no-cutouts)\n"
    "                  [--no-cutouts]    OBJ scenes: ignore map_d images (no alpha cut-outs)   [--kd-alpha]   a 32-bit map_Kd without a map_d is its material's opacity map too\n"
    "                  [--no-normal-maps] OBJ scenes: ignore norm images (--no-textures implies it)   [--bump-as-normal | --bump-height S]   map_Bump / bump as a normal map / a height map of strength S\n"
    "                  [--normal-flip-y]  DirectX-style normal maps: negate green on load\n"
    "                  [--no-spec-maps]   OBJ scenes: ignore map_Ks / map_Pr / map_Pm images (--no-textures implies it)\n"
    "                  [--no-emission-maps] OBJ scenes: ignore map_Ke images (--no-textures implies it)\n"
    "                  [--env FILE [--env-res N] [--env-yaw DEG] [--env-scale S] [--env-hidden]] [--sky R,G,B]   environment lighting\n"
    "                  [--aperture R [--focus D | --focus-pixel X,Y]]   thin-lens camera: depth of field (path tracer)\n"
    "                  [--gpus N [--devices 0,1,..] [--gather rccl|copy]]\n";

int main(int argc, char** argv) {
    std::string scene = "cornell", out, objs, mtl = "./";
    UINT w = 1920, h = 1080, spp = 1, frames = 1, bounces = 8, nee = 1; int device = 0; bool lambert = false;
    int gpus = 1; std::string devlist, gather = "rccl", mode = "pt"; bool literal = false, nee_set = false, bounces_set = false, force_gather = false; float orbit = 0.0f, spin = 0.0f; int only_rank = -1; UINT halo = 0;
    std::vector<UINT> hide; int blink = -1;
    bool adaptive = false; rtx_adaptive ad{}; ad.min_spp = 8; ad.step_spp = 8;
    bool denoise = false; rtx_denoise_params dnp{};
    bool denoise_var = false; float sigma_var = 0.0f; bool sigma_var_set = false;
    bool textures = true; SceneCutouts cutouts = kCutoutsMapD; bool kd_alpha = false; SceneNormals normals; bool no_normals = false, spec_maps = true, emission_maps = true;
    float aperture = 0.0f, focus = 0.0f; bool focus_set = false; std::string focus_pixel;
    std::string env_file, sky; UINT env_res = 512; float env_yaw = 0.0f, env_scale = 1.0f; bool env_hidden = false;
    for (int i = 1; i < argc; i++) {
        auto arg = [&](const char* k) { return !strcmp(argv[i], k) && i + 1 < argc; };
        if (arg("--scene")) scene = argv[++i]; else if (arg("--obj")) { objs = argv[++i]; scene = "obj"; } else if (arg("--mtl")) mtl = argv[++i];
        else if (arg("--w")) w = atoi(argv[++i]); else if (arg("--h")) h = atoi(argv[++i]); else if (arg("--spp")) spp = atoi(argv[++i]);
        else if (arg("--frames")) frames = atoi(argv[++i]); else if (arg("--bounces")) { bounces = atoi(argv[++i]); bounces_set = true; } else if (arg("--nee")) { nee = atoi(argv[++i]); nee_set = true; }
        else if (arg("--mode")) mode = argv[++i]; else if (arg("--orbit")) orbit = (float)atof(argv[++i]); else if (arg("--spin")) spin = (float)atof(argv[++i]); else if (arg("--only-rank")) only_rank = atoi(argv[++i]); else if (!strcmp(argv[i], "--literal")) literal = true; else if (!strcmp(argv[i], "--force-gather")) force_gather = true;
        else if (arg("--hide")) { std::stringstream ss(argv[++i]); std::string t; while (std::getline(ss, t, ',')) hide.push_back((UINT)atoi(t.c_str())); } else if (arg("--blink")) blink = atoi(argv[++i]);
        else if (arg("--adaptive")) { adaptive = true; ad.threshold = (float)atof(argv[++i]); } else if (arg("--min-spp")) ad.min_spp = (uint32_t)atoi(argv[++i]); else if (arg("--step-spp")) ad.step_spp = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--help") || !strcmp(argv[i], "-h")) { fputs(kUsage, stdout); return 0; }
        else if (!strcmp(argv[i], "--no-textures")) textures = false; else if (!strcmp(argv[i], "--no-cutouts")) cutouts = kCutoutsOff; else if (!strcmp(argv[i], "--kd-alpha")) kd_alpha = true;
        else if (!strcmp(argv[i], "--no-spec-maps")) spec_maps = false;
        else if (!strcmp(argv[i], "--no-emission-maps")) emission_maps = false;
        else if (!strcmp(argv[i], "--no-normal-maps")) no_normals = true; else if (!strcmp(argv[i], "--normal-flip-y")) normals.flipY = true;
        else if (!strcmp(argv[i], "--bump-as-normal")) normals.mode = kNormalsBumpAsNormal; else if (arg("--bump-height")) { normals.strength = (float)atof(argv[++i]); normals.mode = kNormalsBumpHeight; }
        else if (arg("--env")) env_file = argv[++i]; else if (arg("--env-res")) env_res = (UINT)atoi(argv[++i]); else if (arg("--env-yaw")) env_yaw = (float)atof(argv[++i]);
        else if (arg("--env-scale")) env_scale = (float)atof(argv[++i]); else if (!strcmp(argv[i], "--env-hidden")) env_hidden = true; else if (arg("--sky")) sky = argv[++i];
        else if (!strcmp(argv[i], "--denoise-albedo")) dnp.flags |= RTX_DENOISE_ALBEDO; else if (!strcmp(argv[i], "--denoise-mapped-normals")) dnp.flags |= RTX_DENOISE_MAPPED_NORMALS;
        else if (!strcmp(argv[i], "--denoise-variance")) denoise_var = denoise = true; else if (arg("--sigma-var")) { sigma_var = (float)atof(argv[++i]); sigma_var_set = true; }
        else if (!strcmp(argv[i], "--denoise")) denoise = true; else if (arg("--denoise-levels")) dnp.levels = (uint32_t)atoi(argv[++i]); else if (arg("--sigma-color")) dnp.sigma_color = (float)atof(argv[++i]); else if (arg("--sigma-plane")) dnp.sigma_plane = (float)atof(argv[++i]);
        else if (arg("--aperture")) aperture = (float)atof(argv[++i]); else if (arg("--focus")) { focus = (float)atof(argv[++i]); focus_set = true; } else if (arg("--focus-pixel")) focus_pixel = argv[++i];
        else if (arg("--halo")) halo = (UINT)atoi(argv[++i]); else if (arg("--gpus")) gpus = atoi(argv[++i]); else if (arg("--devices")) devlist = argv[++i]; else if (arg("--gather")) gather = argv[++i];
        else if (arg("--out")) out = argv[++i]; else if (arg("--device")) device = atoi(argv[++i]); else if (!strcmp(argv[i], "--lambert")) lambert = true;
        else { fprintf(stderr, "unknown argument %s\n", argv[i]); return 2; }
    }
    if (kd_alpha && cutouts != kCutoutsOff) cutouts = kCutoutsKdAlpha;
    if (no_normals) normals.mode = kNormalsOff;
    if (mode != "pt" && mode != "restir") { fprintf(stderr, "--mode must be pt or restir\n"); return 2; }
    const bool restir = mode == "restir";
    if (restir) { if (!nee_set) nee = 4; if (!bounces_set) bounces = 3; }
    if (adaptive && (restir || gpus > 1 || !devlist.empty())) { fprintf(stderr, "--adaptive is the path tracer on one GPU (no --mode restir, --gpus, --devices)\n"); return 2; }
    if (dnp.flags && !denoise) { fprintf(stderr, "--denoise-albedo and --denoise-mapped-normals are options of --denoise\n"); return 2; }
    if (sigma_var_set && !denoise_var) { fprintf(stderr, "--sigma-var is an option of --denoise-variance\n"); return 2; }
    if (denoise_var && (!adaptive || gpus > 1 || !devlist.empty())) { fprintf(stderr, "--denoise-variance needs --adaptive T (the sampler's half sums; T = 0 for a fixed --spp) on one GPU (no --gpus, --devices)\n"); return 2; }
    if (denoise && restir) { fprintf(stderr, "--denoise filters the path tracer's accumulation (no --mode restir: that frame has its own reuse passes)\n"); return 2; }
    if (!env_file.empty() && !sky.empty()) { fprintf(stderr, "--env and --sky exclude each other\n"); return 2; }
    UINT fpx = 0, fpy = 0;
    if (!focus_pixel.empty()) { char tail = 0; if (sscanf(focus_pixel.c_str(), "%u,%u%c", &fpx, &fpy, &tail) != 2) { fprintf(stderr, "--focus-pixel takes X,Y\n"); return 2; } }
    if (aperture > 0.0f && !focus_set && focus_pixel.empty()) { fprintf(stderr, "--aperture needs --focus D or --focus-pixel X,Y\n"); return 2; }
    // the lens of the run, once the camera is in place: autofocus reports its distance; an explicit --focus wins.  measure(x, y) = rtx_focus_distance_at
    auto lens_focus = [&](const std::function<float(UINT, UINT)>& measure) {
        if (!focus_pixel.empty()) {
            const float d = measure(fpx, fpy);
            printf("autofocus: pixel %u,%u is at view depth %.9g%s\n", fpx, fpy, d, d > 0.0f ? "" : " (nothing there)");
            if (!focus_set) focus = d;
        }
        if (aperture > 0.0f && !(focus > 0.0f)) throw std::runtime_error("nothing to focus on: give --focus D or another --focus-pixel");
        return focus;
    };
    SceneEnvironment env;
    try {
        if (!env_file.empty()) env = LoadEnvironment(env_file, env_res, env_yaw, env_scale, env_hidden);
        else if (!sky.empty()) {
            float c[3]; char tail = 0;
            if (sscanf(sky.c_str(), "%f,%f,%f%c", &c[0], &c[1], &c[2], &tail) != 3) { fprintf(stderr, "--sky takes R,G,B\n"); return 2; }
            env = MakeSkyEnvironment(c[0], c[1], c[2]); env.scale = env_scale; env.flags = env_hidden ? RTX_ENV_HIDDEN : 0u;
        }
    } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    // camera of frame f: the scene's eye rotated by f * orbit degrees about the vertical axis through the look-at point
    auto orbit_eye = [&](const Scene& sc, UINT f) {
        const float a = orbit * 3.14159265f / 180.0f * (float)f, cs = cosf(a), sn = sinf(a);
        const float dx = sc.eye.x - sc.center.x, dz = sc.eye.z - sc.center.z;
        return XMFLOAT3(sc.center.x + cs * dx + sn * dz, sc.eye.y, sc.center.z - sn * dx + cs * dz);
    };
    // instance 1 at frame f: its start-up matrix turned by f * spin degrees about the vertical axis (row-vector convention: M * R)
    auto spun = [&](const Scene& sc, UINT f) { return sc.instances[1].transform * XMMatrixRotationAxis({0.f, 1.f, 0.f}, spin * 3.14159265f / 180.0f * (float)f); };
    auto write_image = [&](const std::vector<float>& acc, const std::vector<uint8_t>& px) {
        const bool exr = out.size() > 4 && out.substr(out.size() - 4) == ".exr", png = out.size() > 4 && out.substr(out.size() - 4) == ".png";
        return exr ? WriteEXR(out, acc.data(), w, h) : png ? WritePNG(out, px.data(), w, h) : WritePPM(out, px.data(), w, h);
    };
    if (gpus > 1 || !devlist.empty()) {          // ---- native N-GPU frame (also `--gpus 1 --devices 0`: the same code path with one rank): one process, N contexts on N threads, one all-gather per frame ----
        try {
            std::vector<int> devs;
            if (devlist.empty()) for (int k = 0; k < gpus; k++) devs.push_back(k);
            else { std::stringstream ss(devlist); std::string t; while (std::getline(ss, t, ',')) devs.push_back(atoi(t.c_str())); }
            if ((int)devs.size() != gpus) { fprintf(stderr, "--devices must list %d ordinals\n", gpus); return 2; }
            Scene sc = scene == "cornell" ? MakeCornellBox() : scene == "sponza" ? MakeSponzaClass() : scene == "bistro" ? MakeBistroClass() : Scene();
            if (scene == "obj") { std::vector<std::string> f; std::stringstream ss(objs); std::string t; while (std::getline(ss, t, ',')) f.push_back(t); sc = LoadObjScene(f, mtl, textures, cutouts, normals, spec_maps, emission_maps); }
            if (scene == "cornell") lambert = true;
            if (env.n) sc.environment = env;
            MultiGpuFrame mg(devs, gather == "copy" ? MultiGpuFrame::Gather::COPY : MultiGpuFrame::Gather::RCCL, force_gather, only_rank);      // --force-gather: the collective also with one rank
            mg.SetScene(sc, (float)w / (float)h);
            mg.Clear(w, h);
            for (UINT i : hide) mg.SetInstanceVisible(i, false);
            if (aperture > 0.0f || !focus_pixel.empty()) { const float fd = lens_focus([&](UINT x, UINT y) { return mg.FocusDistanceAt(x, y, only_rank >= 0 ? only_rank : 0); }); mg.SetLens(aperture, fd); }
            bool blink_hidden = blink >= 0 && std::find(hide.begin(), hide.end(), (UINT)blink) != hide.end();
            rtx_params p{}; p.width = w; p.height = h; p.spp = spp; p.max_bounces = bounces; p.nee_samples = nee; p.rr_start = 3;
            p.tile_size = gpus > 1 ? 32 : 64;      // round-robin deal: 32-px tiles even out the background across 8 ranks (max / mean 1.04 instead of 1.15, tools/shard_time.py)
            p.flags = lambert ? RTX_FLAG_LAMBERT_ONLY : (scene == "bistro" ? RTX_FLAG_TRANSMISSION : 0);
            if (restir) { p.spp = 1; p.flags = (lambert ? RTX_FLAG_LAMBERT_ONLY : 0u) | RTX_FLAG_BLOCK_TILES; p.tile_size = 32; mg.SetOption(RTX_OPT_RESTIR_WAVEFRONT, literal ? 0 : 1); mg.ResetRestir(); mg.SetHaloExchange(halo); }
            float prev_view[16] = {0};
            if (spin != 0.0f && sc.instances.size() < 2) { fprintf(stderr, "--spin needs a scene with an instance 1\n"); return 2; }
            for (UINT f = 0; f < frames; f++) {
                p.sample_base = 1 + f * spp; p.frame_seed = f + 1;
                if (spin != 0.0f && f > 0) { mg.SetInstanceTransform(1, spun(sc, f).data()); if (!restir) mg.Clear(w, h); printf("refit on %d ranks: %.3f ms\n", gpus, mg.LastRefitMs()); }
                if (blink >= 0 && f > 0) { blink_hidden = !blink_hidden; mg.SetInstanceVisible((uint32_t)blink, !blink_hidden); if (!restir) mg.Clear(w, h); printf("visibility commit on %d ranks: %.3f ms\n", gpus, mg.LastRefitMs()); }
                if (restir) {
                    nv_helpers_dx12::Manipulator cam; cam.setLookat(orbit_eye(sc, f), sc.center, sc.up);
                    XMMATRIX proj = XMMatrixPerspectiveFovRH(sc.fovY_deg * XM_PI / 180.0f, (float)w / (float)h, sc.zn, sc.zf);
                    mg.SetCamera(cam.getMatrix(), proj.data());
                    if (f == 0) mg.SetCamera(cam.getMatrix(), proj.data());            // previous view = current view for the first frame
                    bool moved = false;                                                // the reference's accumulation reset (RayGen_v6_pass3.hlsl:407-423), as Renderer::UpdateCameraBuffer applies it
                    for (int k = 0; k < 16 && f > 0; k++) moved = moved || fabsf(cam.getMatrix()[k] - prev_view[k]) > 0.00002f;
                    if (moved) mg.Clear(w, h);
                    memcpy(prev_view, cam.getMatrix(), 64);
                    mg.RenderRestir(p);
                } else mg.Render(p);
                double rays = 0; for (int r = 0; r < gpus; r++) { if (only_rank >= 0 && r != only_rank) continue; rtx_stats s = mg.Stats(r); rays += (double)(s.rays_primary + s.rays_extension + s.rays_shadow); }
                printf("frame %u on %d GPUs: %.3f ms (gather included), %.1f Mrays/s\n", f, gpus, mg.LastFrameMs(), rays / (mg.LastFrameMs() * 1e3));
                if (restir && gpus > 1) printf("  history exchange: %s, %.2f MB sent by the busiest rank, stale history reads %llu\n", halo ? "border strips (halo)" : "all-gather", (double)mg.LastExchangeBytes() / 1e6, (unsigned long long)mg.StaleHistoryReads());
            }
            const int rr = only_rank >= 0 ? only_rank : 0;
            if (denoise) { mg.Denoise(&dnp, rr); printf("denoised on rank %d\n", rr); }
            if (denoise && !out.empty()) { if (!write_image(mg.ReadDenoised(rr), mg.ReadDenoisedOutput(rr))) { fprintf(stderr, "error: could not write %s\n", out.c_str()); return 1; } }
            else if (!out.empty() && !write_image(mg.ReadAccumulation(rr), mg.ReadOutput(rr))) { fprintf(stderr, "error: could not write %s\n", out.c_str()); return 1; }
        } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
        return 0;
    }
    try {
        Renderer r(w, h, "rtx_render");
        r.SetDevice(device);
        if (scene == "cornell") { r.SetScene(MakeCornellBox()); lambert = true; }
        else if (scene == "sponza") r.SetScene(MakeSponzaClass());
        else if (scene == "bistro") r.SetScene(MakeBistroClass());
        else { std::vector<std::string> f; std::stringstream ss(objs); std::string t; while (std::getline(ss, t, ',')) f.push_back(t); r.SetLoadTextures(textures); r.SetCutouts(cutouts); r.SetNormalMaps(normals.mode, normals.strength, normals.flipY); r.SetSpecMaps(spec_maps); r.SetEmissionMaps(emission_maps); r.SetModels(f, mtl); }
        if (env.n) r.SetEnvironment(env);
        r.Params().spp = spp; r.Params().max_bounces = bounces; r.Params().nee_samples = nee; r.Params().flags = lambert ? RTX_FLAG_LAMBERT_ONLY : (scene == "bistro" ? RTX_FLAG_TRANSMISSION : 0);
        if (restir) {
            r.SetMode(Renderer::Mode::ReSTIR);
            r.RestirParams().nee_samples = nee; r.RestirParams().max_bounces = bounces; r.RestirParams().flags = lambert ? RTX_FLAG_LAMBERT_ONLY : 0u;
        }
        r.OnInit();
        if (restir && rtx_set_option(r.Context(), RTX_OPT_RESTIR_WAVEFRONT, literal ? 0 : 1) != RTX_OK) throw std::runtime_error(rtx_last_error(r.Context()));
        for (UINT i : hide) r.SetInstanceVisible(i, false);
        if (aperture > 0.0f || !focus_pixel.empty()) { const float fd = lens_focus([&](UINT x, UINT y) { return r.FocusDistanceAt(x, y); }); r.SetLens(aperture, fd); }
        bool blink_hidden = blink >= 0 && std::find(hide.begin(), hide.end(), (UINT)blink) != hide.end();
        XMFLOAT3 eye0, ctr0, up0; nv_helpers_dx12::CameraManip.getLookat(eye0, ctr0, up0);
        Scene inst0; bool have_inst0 = false;
        for (UINT f = 0; f < frames; f++) {
            if (spin != 0.0f && f > 0) {
                if (!have_inst0) { inst0 = scene == "cornell" ? MakeCornellBox() : scene == "sponza" ? MakeSponzaClass() : scene == "bistro" ? MakeBistroClass() : Scene(); if (scene == "obj") { std::vector<std::string> fl; std::stringstream ss(objs); std::string t; while (std::getline(ss, t, ',')) fl.push_back(t); inst0 = LoadObjScene(fl, mtl, false); } have_inst0 = true; }
                if (inst0.instances.size() < 2) { fprintf(stderr, "--spin needs a scene with an instance 1\n"); return 2; }
                r.SetInstanceTransform(1, spun(inst0, f));
                if (!restir) rtx_clear_accum(r.Context(), w, h);               // a moved scene restarts the progressive accumulation (the ReSTIR frame reprojects instead)
            }
            if (orbit != 0.0f) { Scene tmp; tmp.eye = eye0; tmp.center = ctr0; tmp.up = up0; nv_helpers_dx12::CameraManip.setLookat(orbit_eye(tmp, f), ctr0, up0); }
            const bool blinked = blink >= 0 && f > 0;
            if (blinked) { blink_hidden = !blink_hidden; r.SetInstanceVisible((UINT)blink, !blink_hidden); if (!restir) rtx_clear_accum(r.Context(), w, h); }
            r.OnUpdate(); r.Params().sample_base = 1 + f * spp;
            if (adaptive) {                                     // --spp is the cap; a frame after the first continues the image only if the cap grows, so each frame starts afresh
                rtx_params ap = r.Params(); ap.frame_seed = f + 1; ad.max_spp = spp;
                rtx_adaptive_result res{};
                if (f > 0) rtx_clear_accum(r.Context(), w, h);
                if (rtx_render_adaptive(r.Context(), &ap, &ad, &res) != RTX_OK) throw std::runtime_error(std::string("rtx_render_adaptive: ") + rtx_last_error(r.Context()));
                printf("adaptive: threshold %g, min %u / step %u / max %u spp: %u passes, %u chunks (%u converged, %u at max), %llu pixel-samples = %.2f spp on average\n", ad.threshold, ad.min_spp, ad.step_spp, ad.max_spp,
                       res.passes, res.chunks, res.chunks_converged, res.chunks_at_max, (unsigned long long)res.pixel_samples, (double)res.pixel_samples / ((double)w * h));
            } else r.OnRender();
            if (blinked) printf("visibility commit: %.3f ms\n", r.LastRefitMs());
            rtx_stats s = r.Stats();
            double rays = (double)(s.rays_primary + s.rays_extension + s.rays_shadow);
            printf("frame %u: %.3f ms, %.1f Mrays/s (primary %llu, extension %llu, shadow %llu)\n", f, s.render_ms, rays / (s.render_ms * 1e3),
                   (unsigned long long)s.rays_primary, (unsigned long long)s.rays_extension, (unsigned long long)s.rays_shadow);
        }
        if (denoise) {
            rtx_denoise_var_params dvp{};
            dvp.levels = dnp.levels; dvp.sigma_var = sigma_var; dvp.sigma_plane = dnp.sigma_plane; dvp.flags = dnp.flags;
            const rtx_denoise_result dr = denoise_var ? r.DenoiseVariance(&dvp) : r.Denoise(&dnp);
            printf(denoise_var ? "denoise (variance-guided): %u levels, %u pixels filtered, %u passed through\n" : "denoise: %u levels, %u pixels filtered, %u passed through\n", dr.levels, dr.pixels_filtered, dr.pixels_passed);
        }
        if (!out.empty()) {
            const bool exr = out.size() > 4 && out.substr(out.size() - 4) == ".exr", png = out.size() > 4 && out.substr(out.size() - 4) == ".png";
            bool ok;
            if (exr) { std::vector<float> acc = denoise ? r.ReadDenoised() : r.ReadAccumulation(); ok = WriteEXR(out, acc.data(), w, h); }
            else { std::vector<uint8_t> px = denoise ? r.ReadDenoisedOutput() : r.ReadOutput(); ok = png ? WritePNG(out, px.data(), w, h) : WritePPM(out, px.data(), w, h); }
            if (!ok) { fprintf(stderr, "error: could not write %s\n", out.c_str()); return 1; }
        }
        r.OnDestroy();
    } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return 1; }
    return 0;
}

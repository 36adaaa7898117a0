// rtx_ctx.hpp — PRIVATE header of the C-ABI's translation units: the context (struct rtx_ctx), the macros every entry point uses and the helpers they share.
//   rtx_api.hip          create / destroy, options, stream, scene inputs, camera, accumulation, reads, statistics, tile pack / unpack, the shard tiling,
//                        and what the render entry points share: render_checks (their preamble) and stats_begin (the one statistics reset)
//   rtx_commit.hip       rtx_commit_scene (host or GPU build, GPU refit), the scene cache, finalise_scene
//   rtx_render.hip       rtx_render (the wavefront path tracer), render_frame and finish_render
//   rtx_adaptive.hip     rtx_render_adaptive: passes of render_frame over the chunks that have not converged
//   rtx_denoise.hip      rtx_denoise, rtx_denoise_variance and the reads of the denoised image
//   rtx_env.hip          environment lighting: rtx_set_environment and its three debug probes
//   rtx_texture.hip      texture maps: rtx_set_mesh_uvs, rtx_set_texture, rtx_set_material_map, rtx_set_ess_table and the sampler's debug probe
//   rtx_restir_api.hip   the ReSTIR frames, their work lists and lanes, the history / halo exchange between shards
//   rtx_debug.hip        the rtx_debug_* entry points, the per-hit probes of the map slots among them (hit_probe)
// Ownership: every resource of a context is a member of an owning type (rtx_devmem.hpp, rtx_staging.hpp), so `delete c` releases it all.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>
#include "../../include/rtx.h"
#include "rtx_kernels.hpp"
#include "rtx_scene_host.hpp"
#include "rtx_build.hpp"
#include "rtx_devmem.hpp"
#include "rtx_staging.hpp"

using namespace rtx;

// (hidden: the helpers shared by the runtime's translation units are not part of librtx_hip.so's exports)
#pragma GCC visibility push(hidden)

struct TimedLaunch { int cls; hipEvent_t a, b; };

struct rtx_ctx {
    StreamLease streams;            // declared FIRST, so destroyed last: memory and events are freed before the streams go back to the pool.  [0] the context's own stream, [1] aux, [2 .. 4] the lanes
    // ---- the context itself (rtx_api.hip) ----
    int device = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    int num_cus = 256;
    std::string err;
    Staging staging;                // the two pinned chunks every copy from / to caller memory passes through (rtx_staging.hpp)
    Events ev;                      // frame begin / end and the pool of kernel timing and stream joins
    std::vector<TimedLaunch> timed; // the timed launches of the last frame (RTX_OPT_KERNEL_TIMING)
    rtx_stats stats{};

    // ---- options: every value rtx_set_option writes (rtx_api.hip) ----
    struct Options {
        bool timing = false;                        // RTX_OPT_KERNEL_TIMING
        bool async = false;                         // RTX_OPT_ASYNC
        int octant_sort = 0;                        // RTX_OPT_OCTANT_SORT (2 = tooling: all keys zero, i.e. the machinery's overhead without a re-ordering)
        int node_stride = 0;                        // RTX_OPT_NODE_STRIDE
        int restir_keys = 1;                        // RTX_OPT_RESTIR_KEYS
        int sample_interleave = 1;                  // RTX_OPT_SAMPLE_INTERLEAVE
        bool trace_counters = false;                // RTX_OPT_TRACE_COUNTERS
        int any_order_opt = -1;                     // RTX_OPT_ANYHIT_ORDER: -1 = what the commit-time probe chose (BuiltScene::any_order)
        uint64_t paths_per_batch = 128u << 20;      // RTX_OPT_PATHS_PER_BATCH
        uint32_t sort_materials = 0;                // RTX_OPT_SORT_MATERIALS
        int lds_nodes_opt = -1;                     // RTX_OPT_LDS_NODES
        int partial_refit = 1;                      // RTX_OPT_PARTIAL_REFIT: partial GPU refit (node_aabb / d_scale hold the last full refit's state)
        int lds_closest_opt = -1;                   // RTX_OPT_LDS_NODES_CLOSEST
        bool small_scene = true;                    // RTX_OPT_SMALL_SCENE
        bool small_slabs = true;                    // RTX_OPT_SMALL_SLABS: near-parallelogram record pairs are pre-tested by two slabs per record (DevScene::small_slab_mask)
        bool fused = true;                          // RTX_OPT_FUSED_BOUNCE
        int bounce_variant = 2;                     // RTX_OPT_BOUNCE_VARIANT: 0 workgroup hit ring, 1 no ring, 2 wave-private rings
        bool shared_primary = true;                 // RTX_OPT_SHARED_PRIMARY
        int stack_private = -1;                     // RTX_OPT_STACK_PRIVATE
        bool lpt_order = true;                      // RTX_OPT_LPT_ORDER: fused kernels take their sub-queues longest first
        bool fused_bvh = false;                     // RTX_OPT_FUSED_BVH: general path = one k_bounce_bvh launch per batch (trace -> shade -> shadow per sub-queue and bounce); measured SLOWER, default off
        bool work_stealing = false;                 // RTX_OPT_WORK_STEALING: trace kernels of general scenes continue with other sub-queues instead of draining (refill_steal); measured SLOWER, default off
        bool compact_state = true;                  // RTX_OPT_COMPACT_STATE: the separate kernels and the fused tiny-scene kernels keep ray / throughput (/ hit) records by queue position, ping-pong (DevPaths::out_*)
        bool overlap_shadow = true;                 // RTX_OPT_OVERLAP_SHADOW: k_trace_shadow of bounce b on a second stream, beside k_trace_closest of bounce b + 1 (not while kernels are timed)
        uint32_t blocks_per_cu = 0;                 // RTX_OPT_BLOCKS_PER_CU (0 = auto)
        bool taper = true; uint32_t taper_levels = 4;   // RTX_OPT_TAPER
        uint32_t merge_rays = 1024;                 // RTX_OPT_MERGE_RAYS
        bool gpu_refit = true;                      // RTX_OPT_GPU_REFIT
        int gpu_build = 0;                          // RTX_OPT_GPU_BUILD
        int deform_rebuild = 0;                     // RTX_OPT_DEFORM_REBUILD: 0 a vertex-changing commit refits, 1 it rebuilds, N >= 2 it rebuilds once the tree's visit cost exceeds N % of its value after the last build
        uint32_t stack_cap = 11;                    // RTX_OPT_STACK_CAP: traversal-stack entries kept in LDS (0 = all of them)
        int shade_dense = 0;                        // RTX_OPT_SHADE_DENSE
        uint32_t occluder_cache = 0;                // RTX_OPT_OCCLUDER_CACHE
        bool restir_wave = true;                    // RTX_OPT_RESTIR_WAVEFRONT
        uint32_t restir_lane_min = 1u << 16;        // RTX_OPT_RESTIR_LANE_MIN: pixel lists shorter than this run as one chain
        uint32_t restir_lanes = 2;                  // RTX_OPT_RESTIR_LANES: the work list of a ReSTIR frame as 1 .. 4 independent parts on as many streams (the tails of one part's many short launches fill with the others' work)
        uint32_t restir_chunks = 4;                 // RTX_OPT_RESTIR_CHUNKS: 256-item chunks per sub-queue (= workgroup) of the ReSTIR stages
        uint32_t trace_sched = 6;                   // RTX_OPT_TRACE_SCHED
        uint32_t refill_min = 12;                   // RTX_OPT_REFILL_MIN
    } opt;                                          // (RTX_OPT_BVH_REINSERT / RTX_OPT_BVH_SPLIT write host.bvh)
    DevBuf d_trace_cnt;                             // RTX_OPT_TRACE_COUNTERS: the counters (allocated when the option is switched on)

    // ---- scene inputs, camera, accumulation (rtx_api.hip) ----
    SceneHost host;
    bool committed = false;                         // cleared by every input or layout option that changes the scene; set by finalise_scene
    float view[16], proj[16], prev_view[16], prev_proj[16]; bool camera_set = false; DevBuf d_cam;
    rtx_lens lens{};                                // rtx_set_lens: camera state beside the matrices (make_frame hands it to the raygen kernels); all zero = the pinhole
    DevBuf d_accum; void* ext_accum = nullptr; size_t ext_accum_bytes = 0; uint32_t acc_w = 0, acc_h = 0;
    DevBuf d_srgb;                                  // rtx_read_srgb8 / rtx_read_layer
    F4* accum_ptr() { return (F4*)(ext_accum ? ext_accum : d_accum.p); }

    // ---- the resident scene (rtx_commit.hip) ----
    DevScene dsc{};                                 // what the kernels read of it: finalise_scene, plus the option values of options_to_scene (rtx_api.hip)
    struct Scene {
        BuiltScene built;
        bool committed_once = false;
        DevBuf d_nodes, d_tris, d_small, d_small_tris, d_small_poly, d_small_slabs, d_shade, d_mats, d_insts, d_lights, d_cdf;
        std::vector<float> h_cdf; std::vector<uint32_t> h_one;     // host sources of small asynchronous uploads
        // the wide tree as the DEVICE holds it (the host mirror B.nodes8 / B.tris8 is empty after a GPU build): counts, the root record (octant-sort grid), who built it
        uint32_t n_nodes8 = 0, n_tris8 = 0; Node8GPU root8{}; bool dev_built = false; std::unique_ptr<GpuBvhBuilder> builder; GpuBuildResult build_info;
        // the meshes as they were handed over, resident on the device (RTX_OPT_GPU_BUILD: from the first commit; a host-built scene: from its first vertex-changing commit).  A
        // commit uploads what was added since the last one and overwrites the vertex ranges named in pool_dirty (rtx_update_mesh_vertices); the per-instance ranges k_flatten
        // reads, and the compacted list of the instances of changed meshes k_reflatten reads (csrc/rtx_build.hip)
        DevBuf d_work_insts; std::vector<FlatInst> h_work; std::vector<uint32_t> pool_dirty;
        bool host_mirror_stale = false;                  // B.shade / B.objtris describe the vertices of an earlier commit (the device re-derived its records from the pool): nothing may read them
        // tree quality (k_tree_cost): per-workgroup partial sums on the device, and their sums once read.  state 0 = not computed for the tree as it is, 1 = enqueued, 2 = read
        DevBuf d_cost_base, d_cost_now; int cost_base_state = 0, cost_now_state = 0; double cost_base = 0.0, cost_now = 0.0;
        DevBuf d_pool_verts, d_pool_idx, d_pool_matids, d_flat_insts; size_t pool_verts = 0, pool_idx = 0, pool_matids = 0, pool_meshes = 0; std::vector<uint32_t> pool_vert_base, pool_idx_base; std::vector<FlatInst> h_flat;
        DevBuf d_inst_hidden;                            // rtx_set_instance_visible: BuiltScene::inst_hidden for the refit kernels (uploaded only while something is hidden)
        DevBuf d_inst_moved, d_tri_dirty, d_node_dirty; bool node_aabb_valid = false;      // partial GPU refit: node_aabb / d_scale hold the last full refit's state
        DevBuf d_objtris, d_node_aabb, d_scale;          // GPU refit: object-space vertices (uploaded on first use), per-node float boxes, max |coordinate|
        bool device_scene_valid = false, objtris_uploaded = false;
        DevBuf d_nodes_wide; bool wide_nodes = false;    // the copy with one node per 128-B line (RTX_OPT_NODE_STRIDE)
        uint32_t lds_nodes_closest = 0;                  // staged nodes of the closest-hit launches (pick_lds_closest)
        DevBuf d_stack_ovf;                              // the traversal stack's overflow columns of deeper trees (RTX_OPT_STACK_CAP)
        // texture maps (sync_textures, rtx_commit.hip): descriptors, the texel pool and the per-material map ids follow the host's tables at every commit that changed them;
        // the byte -> float tables once.  d_mat_maps: ONE int32 table, a row of mat_maps_nmat entries per slot the kernels read by material (every MapSlot but the opacity
        // slot, whose ids are per triangle: d_tri_cut), -1 = no map; finalise_scene points DevScene::map_* at its rows.  The energy table of rtx_set_ess_table only while the
        // host holds one
        DevBuf d_tex_desc, d_texels, d_tex_lut, d_mat_maps, d_ess_tab; uint32_t ntex = 0; size_t mat_maps_nmat = 0;
        static constexpr uint32_t kMatMapRows = kMapSlotCount - 1;
        static uint32_t mat_map_row(MapSlot s) { return s < kMapOpacity ? s : s - 1u; }
        const int32_t* mat_maps(MapSlot s) const { return d_mat_maps.p ? (const int32_t*)d_mat_maps.p + mat_map_row(s) * mat_maps_nmat : nullptr; }
        // the per-triangle tables, by GLOBAL triangle id: tri_uv while any map group is active (BuiltScene::map_use), rebuilt when UVs or the triangle numbering changed;
        // tri_cut while a cut-out is active, rebuilt with it; tri_tan while a normal map is active, rebuilt when UVs, the triangle numbering or a mesh's vertices changed
        // (object space: a transform-only commit leaves it alone); q of the emission maps with the light list, while one is active
        DevBuf d_tri_uv, d_tri_cut, d_tri_tan, d_emi_q; bool tri_uv_valid = false, tri_cut_valid = false, tri_tan_valid = false;
        DevBuf d_lights_plain, d_cdf_plain; std::vector<float> h_cdf_plain;      // ... and the unmapped scene's light list, for the renderers that ignore the maps (plain_scene())
        // environment lighting (sync_environment, rtx_commit.hip): the tables of the bound map, rebuilt by the commit after rtx_set_environment; env_total = their weight sum
        DevBuf d_env_tex, d_env_marg, d_env_cond; double env_total = 0.0;
    } scene;
    // the scene as rtx_render_v6_pass1 and rtx_render_restir read it: they ignore the emission maps (include/rtx.h, EMISSION MAPS), so while one is active they get the
    // light list of the unmapped scene and no emission tables; otherwise dsc as it is
    DevScene plain_scene() const {
        DevScene s = dsc;
        if (scene.built.map_use.emi()) {
            s.lights = (const LightGPU*)scene.d_lights_plain.p; s.cdf = (const float*)scene.d_cdf_plain.p; s.nlights = (uint32_t)scene.built.lights_plain.size();
            s.total_weight = scene.built.total_weight_plain; s.map_ke = nullptr; s.emi_q = nullptr;
        }
        return s;
    }

    // ---- the path tracer's frame (rtx_render.hip) ----
    struct PathFrame {
        DevBuf d_ray_o, d_ray_d, d_thr, d_rad, d_hit, d_sh_o, d_sh_d, d_sh_c, d_queue[2], d_counters;
        DevBuf d_alt_o, d_alt_d, d_alt_thr;              // the second path-state set of the compact state (separate kernels; the fused tiny-scene kernels keep both sets in d_ray_o / d_ray_d / d_thr)
        DevBuf d_hitmask, d_order, d_pmask;
        DevBuf d_prim_rec, d_prim_hits;                  // RTX_OPT_SHARED_PRIMARY: the per-pixel primary surface records and per-block hit masks of the current call (k_primary_surface)
        DevBuf d_oct[2], d_perm;                         // RTX_OPT_OCTANT_SORT
        DevBuf d_hitq;                                   // RTX_OPT_FUSED_BVH
        DevBuf d_heads;                                  // RTX_OPT_WORK_STEALING: per trace launch of a batch, G fetch cursors + the retired count
        PinnedBuf h_counters;                            // the per-batch counters of a frame, read back in one copy each
        // RTX_OPT_MERGE_RAYS: thin launches of the traversal kernels take several sub-queues per workgroup (MergedQ).  The host cannot see a launch's ray count (it is on the
        // device), so it predicts it from the counters of the previous rtx_render of this context: per path entering the batch, how many were still alive at bounce b and how many
        // shadow rays slot j of bounce b cast.  A wrong prediction costs time only.
        uint64_t pred_paths = 0; std::vector<uint64_t> pred_q, pred_s; uint32_t pred_nee1 = 0;
        hipStream_t aux = nullptr;                       // RTX_OPT_OVERLAP_SHADOW: the shadow stream (streams.set.s[1], taken on first use)
        // RTX_OPT_ASYNC: what finish_render needs of the frame that rtx_render enqueued
        struct Pending { bool active = false; size_t ncnt = 0; uint32_t nbatches = 0, G = 0, mb = 0, nee = 0, nee1 = 1; bool fused = false, fused_bvh = false; } pending;
    } pt;

    // ---- adaptive sampling (rtx_adaptive.hip) ----
    struct Adaptive {
        // `half` (W x H, the running sum of the odd-id samples) and per IMAGE chunk — tile t, 256-slot strip k of it: word (t << cs) | k, whichever shard renders it — the samples
        // taken and the sticky flag (AdaptState, rtx_kernels.hpp); the active list of the current pass (local chunk ids of the shard) and the five words read back per pass
        DevBuf d_half, d_count, d_flag, d_list, d_out;
        bool pure = true;               // every sample in u1 since its last clear came from rtx_render_adaptive (rtx_render, rtx_render_v6_pass1 and rtx_render_restir clear this)
        bool cleared = true;            // u1 was cleared since the state above was last used: the next rtx_render_adaptive zeroes it
        uint32_t key[3] = {0, 0, 0};    // width, height, tile size the state is laid out for
        bool whole = true;              // `half` holds the second sum of EVERY pixel of u1: no rtx_render_adaptive since the state was zeroed was sharded and no rtx_unpack_tiles wrote u1 (rtx_denoise_variance needs it)
    } ad;

    // ---- the denoiser (rtx_denoise.hip) ----
    struct Denoise {
        DevBuf d_guides, d_pp[2], d_out, d_partial, d_count;     // 32 B of guides per pixel, the two ping-pong images, the denoised image; per-workgroup counts of the first level and their sum
        DevBuf d_mguides;                                         // 32 B of map guides per pixel (A, nm): allocated by the first call with a flag set
        uint32_t w = 0, h = 0; bool valid = false;                // size of the denoised image; a successful rtx_denoise wrote it
        Events ev;                                                // guides / filter begin and end (RTX_OPT_KERNEL_TIMING), rewound per call
        uint32_t lds_step = 4;                                    // RTX_OPT_DENOISE_LDS_STEP
    } dn;

    // ---- ReSTIR (rtx_restir_api.hip) ----
    struct Restir {
        DevBuf d_res_di, d_res_gi, d_sdata, d_last_di, d_last_gi, d_last_sd, d_p1cnt, d_p1scratch; size_t p1_slots = 0, last_slots = 0;
        DevBuf d_rs_key_a, d_rs_key_b;                   // RTX_OPT_RESTIR_KEYS
        // work lists (x | y << 16 per pixel, 8 x 8 pixel blocks in MORTON order so that consecutive chunks are compact screen regions): the shard's own pixels
        // (pass 3) and — on shards — its tiles dilated by the 20-px radius of the spatial pass (passes 1 and 2); key = (width, height, tile, rank, count, deal)
        DevBuf d_halo, d_own; uint32_t halo_count = 0, own_count = 0; uint32_t halo_key[6] = {0, 0, 0, 0, 0, 0};
        // where this context holds last frame's history (pixel rectangle, exclusive upper bounds): the whole image after a reset / an unsharded frame / rtx_restir_unpack_state,
        // the own rectangle after a sharded frame, + halo_px after rtx_restir_unpack_halo; hist_all = the whole image whatever its size
        uint32_t hist[4] = {0, 0, 0, 0}; bool hist_all = true;
        // wavefront ReSTIR (rtx_restir_wave.hpp): path state by queue position (two sets), hit records, per-item records, the any-hit ray queue, queue lengths
        struct RsArea { DevBuf state, hit, cls, fin, cold, occ, cand, sho, shd, pay, cnt; } rs_area[4];      // one per pipeline lane (RTX_OPT_RESTIR_LANES)
        hipStream_t lane_stream[3] = {nullptr, nullptr, nullptr};      // lanes 1 .. 3 (lane 0 runs on the context's stream): streams.set.s[2 ..], taken on first use
    } rs;
};

// message of the calls that have no context to hold one (rtx_create failing, rtx_shard_slab_bytes, rtx_restir_state_slab_bytes, rtx_restir_halo_plan): PER THREAD, so the N threads
// of the native multi-GPU frame (host/MultiGpu.cpp) that ask for their slab sizes at once never write the same string; rtx_last_error(NULL) reads the caller's own
extern thread_local std::string g_create_err;

#define HIPCHK(c, call)                                                                          \
    do { hipError_t e_ = (call);                                                                 \
         if (e_ != hipSuccess) { (c)->err = std::string(#call) + ": " + hipGetErrorString(e_);  \
                                 return e_ == hipErrorOutOfMemory ? RTX_ERR_OOM : RTX_ERR_HIP; } } while (0)
// RTX_OPT_ASYNC: an rtx_render that only ENQUEUED its frame leaves statistics to be collected (finish_render: stream sync + counter read-back).  Every entry point joins
// first (BIND) — except the calls a frame's epilogue is made of, which must stay stream-ordered behind the render without a host join (BIND_NOWAIT: pack / unpack)
int finish_render(rtx_ctx* c);
void collect_timed(rtx_ctx* c);
// a pass of rtx_render_adaptive for render_frame (rtx_render.hip): the active list (local chunk ids, ascending), the first sample id, the state the accumulation updates;
// first: the per-call tables of the tiny-scene path (packet masks / shared primary records) are still to be computed
struct ListPass { const uint32_t* list; uint32_t n_active, sample_first; AdaptState state; bool first; };
int render_frame(rtx_ctx* c, const rtx_params* p, const DevFrame& f_real, uint32_t spp, const ListPass* lp);
#define BIND_NOWAIT(c) do { if (!(c)) return RTX_ERR_INVALID; HIPCHK(c, hipSetDevice((c)->device)); } while (0)
#define BIND(c) do { BIND_NOWAIT(c); if ((c)->pt.pending.active) { const int r_ = finish_render(c); if (r_ != RTX_OK) return r_; } } while (0)

// EVERY copy between host arrays and the device goes through these two (rtx_staging.hpp: pinned chunks of the context).  to_device: the source is consumed when it returns
// and the copy is ordered on the context's stream — no lifetime rule, no synchronise.  to_host: complete when it returns (it waits for the stream up to the copy).
#define TO_DEVICE(c, dst, src, bytes) HIPCHK(c, (c)->staging.to_device((c)->stream, (dst), (src), (bytes)))
#define TO_HOST(c, dst, src, bytes) HIPCHK(c, (c)->staging.to_host((c)->stream, (dst), (src), (bytes)))
template <class T> static int upload(rtx_ctx* c, DevBuf& b, const std::vector<T>& v) {
    HIPCHK(c, b.ensure(v.size() * sizeof(T)));
    TO_DEVICE(c, b.p, v.data(), v.size() * sizeof(T));
    return RTX_OK;
}

// one launch of kernel class `cls`: counted, and timed between two events of the pool while RTX_OPT_KERNEL_TIMING is on
struct Timed {
    rtx_ctx* c; int cls; hipEvent_t a = nullptr, b = nullptr;
    hipStream_t s;
    Timed(rtx_ctx* c_, int cls_, hipStream_t s_ = nullptr) : c(c_), cls(cls_), s(s_ ? s_ : c_->stream) { c->stats.kernel_launches[cls]++; if (c->opt.timing) { a = c->ev.take(); b = c->ev.take(); if (a) (void)hipEventRecord(a, s); } }
    ~Timed() { if (c->opt.timing && a && b) { (void)hipEventRecord(b, s); c->timed.push_back({cls, a, b}); } }
};

// rtx_api.hip
void options_to_scene(rtx_ctx* c, bool committed);
int render_checks(rtx_ctx* c, const rtx_params* p, bool zero_bounces_ok, DevFrame& f);    // the preamble of every render entry point: context, scene, camera, frame, limits
void stats_begin(rtx_ctx* c);
int ensure_accum(rtx_ctx* c, uint32_t w, uint32_t h, bool clear);
const char* validate_tiling(const rtx_params* p, uint32_t& ts, uint32_t& cnt, uint64_t& npl, uint32_t* gx_out = nullptr, uint32_t* gy_out = nullptr);
int make_frame(rtx_ctx* c, const rtx_params* p, DevFrame& f);
void block_rect(uint32_t W, uint32_t H, uint32_t ts, uint32_t TX, uint32_t TY, uint32_t gx, uint32_t gy, uint32_t r, uint32_t out[4]);
// rtx_commit.hip
void pick_lds_closest(rtx_ctx* c);
int tree_costs(rtx_ctx* c, double out2[2]);     // {visit cost of the resident tree now, after its last build}; RTX_ERR_STATE for a tree the GPU refit does not handle

#pragma GCC visibility pop

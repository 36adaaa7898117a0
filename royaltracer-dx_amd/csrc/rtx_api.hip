// rtx_api.hip — the C-ABI of include/rtx.h: the context, its options and stream, scene inputs, camera, accumulation, image reads, statistics, the shard tiling.
// Host code only (kernels: the headers rtx_kernels.hip includes, and rtx_refit.hip).  No CPU rendering path exists here by design.  The context and the other parts of the C-ABI: rtx_ctx.hpp.
#include "rtx_ctx.hpp"
#include <cmath>

thread_local std::string g_create_err;

// the option values the kernels read, copied into DevScene: after rtx_set_option changed one of them, and by finalise_scene.  The any-hit order only on a committed
// scene (`committed`): -1 takes what the commit-time probe chose.
void options_to_scene(rtx_ctx* c, bool committed) {
    DevScene& s = c->dsc; const rtx_ctx::Options& o = c->opt;
    s.trace_cnt = o.trace_counters ? (unsigned long long*)c->d_trace_cnt.p : nullptr;
    s.refill_min = o.refill_min; s.trace_sched = o.trace_sched; s.sort_materials = o.sort_materials; s.occluder_cache = o.occluder_cache; s.shade_dense = o.shade_dense > 0 ? 1u : 0u;
    if (committed) {
        s.any_order = o.any_order_opt < 0 ? c->scene.built.any_order : (uint32_t)o.any_order_opt;
        s.any_order_occ = o.any_order_opt < 0 ? 0u : (uint32_t)o.any_order_opt;
        s.small_slab_mask = o.small_slabs ? c->scene.built.small_slab_mask : 0u;      // 0: every pair generic — the same kernels, their wave-uniform branch never taken
    }
}

// What every render entry point checks first, in this order: the context (joining a frame left in flight), the committed scene, the camera, the frame of `p`, the limits.
// zero_bounces_ok: false = the path tracer (rtx_render, rtx_render_adaptive: max_bounces in [1, 64]), true = the ReSTIR entry points (pass 1 alone is a frame: [0, 64]);
// the two kinds of call also word the error differently.  Touches no image and no state.
int render_checks(rtx_ctx* c, const rtx_params* p, bool zero_bounces_ok, DevFrame& f) {
    BIND(c);
    if (!c->committed) { c->err = "render: scene not committed"; return RTX_ERR_STATE; }
    if (!c->camera_set) { c->err = "render: camera not set"; return RTX_ERR_STATE; }
    const int r = make_frame(c, p, f);
    if (r) return r;
    if (zero_bounces_ok) {
        if (p->max_bounces > 64 || p->nee_samples > 16) { c->err = "params: max_bounces <= 64, nee_samples <= 16"; return RTX_ERR_INVALID; }
        return RTX_OK;
    }
    if (p->max_bounces == 0 || p->max_bounces > 64) { c->err = "params: max_bounces must be in [1, 64]"; return RTX_ERR_INVALID; }
    if (p->nee_samples > 16) { c->err = "params: nee_samples must be <= 16"; return RTX_ERR_INVALID; }
    return RTX_OK;
}
// the one reset of a frame's statistics (stats_end_restir / finish_render fill them in) and of the timing events: the union of what the entry points used to reset
void stats_begin(rtx_ctx* c) {
    memset(c->stats.kernel_ms, 0, sizeof(c->stats.kernel_ms));
    memset(c->stats.kernel_launches, 0, sizeof(c->stats.kernel_launches));
    memset(c->stats.kernel_items, 0, sizeof(c->stats.kernel_items));
    c->stats.rays_primary = c->stats.rays_extension = c->stats.rays_shadow = c->stats.paths = c->stats.primary_hits = 0; c->stats.render_ms = 0;
    c->ev.used = 0; c->timed.clear();
}

int ensure_accum(rtx_ctx* c, uint32_t w, uint32_t h, bool clear) {
    const size_t need = (size_t)w * h * 16;
    if (c->ext_accum) {
        if (c->ext_accum_bytes < need) { c->err = "bound accumulation buffer is smaller than width*height*16 bytes"; return RTX_ERR_INVALID; }
    } else {
        const bool fresh = !c->d_accum.p || c->acc_w != w || c->acc_h != h;
        HIPCHK(c, c->d_accum.ensure(need));
        clear = clear || fresh;
    }
    c->acc_w = w; c->acc_h = h;
    if (clear) { HIPCHK(c, hipMemsetAsync(c->accum_ptr(), 0, need, c->stream)); c->ad.pure = true; c->ad.cleared = true; }      // (the adaptive state is zeroed by the call that next uses it)
    return RTX_OK;
}

// the ONE rule for the shard tiling, shared by every entry point that takes rtx_params (render, pack / unpack, rtx_shard_slab_bytes):
// tile_size a power of two in [16, 1024] (0 => 64), shard_rank < shard_count, the local slot count fits 31 bits.  All in 64-bit arithmetic.
// RTX_FLAG_BLOCK_TILES: the ranks form a gx x gy grid of tile rectangles, gx gy = shard_count with the smallest rectangle perimeter; on a TIE the
// first factorisation in ascending gx wins, i.e. the grid with FEWER columns (taller).  royaltracer-dx_amd/sharding.py block_grid mirrors this loop line for line — pack / unpack and the slab
// sizes of all ranks depend on both sides agreeing, so change them together (tests/test_multigpu_gloo.py::test_block_grid_tie_goes_to_the_grid_with_fewer_columns pins the choice).
static void block_grid(uint64_t TX, uint64_t TY, uint32_t N, uint32_t& gx, uint32_t& gy) {
    double best = 1e300; gx = N; gy = 1;
    for (uint32_t a = 1; a <= N; a++) {
        if (N % a) continue;
        const uint32_t b = N / a;
        const double cost = (double)((TX + a - 1) / a) + (double)((TY + b - 1) / b);
        if (cost < best) { best = cost; gx = a; gy = b; }
    }
}
const char* validate_tiling(const rtx_params* p, uint32_t& ts, uint32_t& cnt, uint64_t& npl, uint32_t* gx_out, uint32_t* gy_out) {
    if (!p || !p->width || !p->height) return "params: width/height must be non-zero";
    ts = p->tile_size ? p->tile_size : 64;
    if (ts < 16 || ts > 1024 || (ts & (ts - 1))) return "params: tile_size must be a power of two in [16, 1024] (0 = 64)";
    cnt = p->shard_count ? p->shard_count : 1;
    if (p->shard_rank >= cnt) return "params: shard_rank >= shard_count";
    const uint64_t TX = (p->width + (uint64_t)ts - 1) / ts, TY = (p->height + (uint64_t)ts - 1) / ts;
    uint64_t per = (TX * TY + cnt - 1) / cnt;
    uint32_t gx = 0, gy = 0;
    if ((p->flags & RTX_FLAG_BLOCK_TILES) && cnt > 1) { block_grid(TX, TY, cnt, gx, gy); per = ((TX + gx - 1) / gx) * ((TY + gy - 1) / gy); }
    if (gx_out) *gx_out = gx;
    if (gy_out) *gy_out = gy;
    if (per > 0x7FFFFFFFull / ((uint64_t)ts * ts)) return "params: image too large";      // (checked before the multiplication: 2^56 tiles of 16 x 16 would wrap)
    npl = per * ts * ts;
    return nullptr;
}

int make_frame(rtx_ctx* c, const rtx_params* p, DevFrame& f) {
    uint32_t ts = 0, cnt = 0; uint64_t npl64 = 0;
    if (const char* e = validate_tiling(p, ts, cnt, npl64, &f.blk_gx, &f.blk_gy)) { c->err = e; return RTX_ERR_INVALID; }
    f.width = p->width; f.height = p->height; f.tile_size = ts;
    f.tile_shift = 0; while ((1u << f.tile_shift) < ts) f.tile_shift++;
    f.nblocks = 1; f.qcap = 0; f.chunks_per_sample = 0; f.taper_levels = 0; f.interleave = 0;
    f.tiles_x = (p->width + ts - 1) / ts; f.tiles_y = (p->height + ts - 1) / ts;
    f.shard_rank = p->shard_rank; f.shard_count = cnt;
    f.npl = (uint32_t)npl64;
    f.chunks_per_sample = f.npl / 256;          // tile_size >= 16 makes npl a multiple of 256
    f.batch_spp = 1; f.sample_first = p->sample_base;
    f.max_bounces = p->max_bounces; f.nee_samples = p->nee_samples; f.rr_start = p->rr_start;
    f.frame_seed = p->frame_seed; f.flags = p->flags;
    f.hist_x0 = f.hist_y0 = 0; f.hist_x1 = p->width; f.hist_y1 = p->height; f.hist_stale = nullptr;
    f.list = nullptr;
    f.lens_radius = c->lens.aperture_radius; f.lens_focus = c->lens.focus_distance;
    return RTX_OK;
}
// pixel rectangle [x0, x1) x [y0, y1) of rank r in the RTX_FLAG_BLOCK_TILES deal (shard_tile's rule, clipped to the image)
void block_rect(uint32_t W, uint32_t H, uint32_t ts, uint32_t TX, uint32_t TY, uint32_t gx, uint32_t gy, uint32_t r, uint32_t out[4]) {
    const uint32_t bx = r % gx, by = r / gx;
    out[0] = std::min(W, (bx * TX / gx) * ts); out[2] = std::min(W, ((bx + 1u) * TX / gx) * ts);
    out[1] = std::min(H, (by * TY / gy) * ts); out[3] = std::min(H, ((by + 1u) * TY / gy) * ts);
}

extern "C" {

int rtx_create(int device_ordinal, rtx_ctx** out) {
    if (!out) return RTX_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_create_err = std::string("no HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                       " (this library has no CPU fallback)";
        return RTX_ERR_NO_DEVICE;
    }
    if (device_ordinal < 0 || device_ordinal >= n) { g_create_err = "device ordinal out of range"; return RTX_ERR_NO_DEVICE; }
    if ((e = hipSetDevice(device_ordinal)) != hipSuccess) { g_create_err = hipGetErrorString(e); return RTX_ERR_NO_DEVICE; }
    rtx_ctx* c = new rtx_ctx();
    c->device = device_ordinal;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) c->num_cus = prop.multiProcessorCount;
    if ((e = c->streams.acquire(device_ordinal)) != hipSuccess) {
        g_create_err = hipGetErrorString(e); delete c; return RTX_ERR_HIP;
    }
    c->stream = c->streams.set.s[0]; c->own_stream = true;
    (void)hipEventCreate(&c->ev.begin); (void)hipEventCreate(&c->ev.end);
    *out = c;
    return RTX_OK;
}

void rtx_destroy(rtx_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    // a caller-owned stream (rtx_set_stream) may already be gone (torch destroys its streams first): every entry point that enqueues on it
    // synchronises before it returns or documents that it only enqueues, so only the context's own stream is drained here
    if (c->own_stream && c->stream) (void)hipStreamSynchronize(c->stream);
    else (void)hipDeviceSynchronize();
    delete c;                       // memory and events (the members' destructors), then the streams go back to the pool (StreamLease, destroyed last)
}

const char* rtx_last_error(rtx_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int rtx_set_option(rtx_ctx* c, int option, int64_t value) {
    if (!c) return RTX_ERR_INVALID;
    switch (option) {
    case RTX_OPT_KERNEL_TIMING: c->opt.timing = value != 0; return RTX_OK;
    case RTX_OPT_ASYNC: c->opt.async = value != 0; return RTX_OK;
    case RTX_OPT_OCTANT_SORT: c->opt.octant_sort = (int)value; return RTX_OK;
    case RTX_OPT_NODE_STRIDE: if (value != 0 && value != 80 && value != 128) { c->err = "node stride must be 0 (auto), 80 or 128"; return RTX_ERR_INVALID; } if (c->opt.node_stride != (int)value) { c->opt.node_stride = (int)value; c->committed = false; } return RTX_OK;
    case RTX_OPT_RESTIR_KEYS: c->opt.restir_keys = value != 0; return RTX_OK;
    case RTX_OPT_SAMPLE_INTERLEAVE: c->opt.sample_interleave = value != 0; return RTX_OK;
    case RTX_OPT_TRACE_COUNTERS:
        c->opt.trace_counters = value != 0;
        if (c->opt.trace_counters) { HIPCHK(c, c->d_trace_cnt.ensure(4 * sizeof(unsigned long long))); HIPCHK(c, hipMemsetAsync(c->d_trace_cnt.p, 0, 32, c->stream)); }
        options_to_scene(c, c->committed);
        return RTX_OK;
    case RTX_OPT_BVH_REINSERT: if (value < 0 || value > 16) { c->err = "bvh_reinsert must be in [0, 16]"; return RTX_ERR_INVALID; } c->host.bvh.reinsert_passes = (int)value; c->host.topo_dirty = true; c->committed = false; return RTX_OK;
    case RTX_OPT_BVH_SPLIT: if (value < 0 || value > 1000000000) { c->err = "bvh_split must be in [0, 1e9] (parts per billion of the scene's surface area)"; return RTX_ERR_INVALID; } c->host.bvh.split_alpha = (double)value * 1e-9; c->host.topo_dirty = true; c->committed = false; return RTX_OK;
    case RTX_OPT_ANYHIT_ORDER: if (value < -1 || value > 2) { c->err = "anyhit_order must be -1 (probe), 0, 1 or 2"; return RTX_ERR_INVALID; } c->opt.any_order_opt = (int)value; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_PATHS_PER_BATCH: if (value < 4096) { c->err = "paths_per_batch must be >= 4096"; return RTX_ERR_INVALID; } c->opt.paths_per_batch = (uint64_t)value; return RTX_OK;
    case RTX_OPT_SORT_MATERIALS: c->opt.sort_materials = value != 0; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_LDS_NODES: c->opt.lds_nodes_opt = (int)value; c->committed = false; return RTX_OK;
    case RTX_OPT_PARTIAL_REFIT: c->opt.partial_refit = value != 0; return RTX_OK;
    case RTX_OPT_LDS_NODES_CLOSEST: c->opt.lds_closest_opt = (int)value; if (c->committed) pick_lds_closest(c); return RTX_OK;
    case RTX_OPT_SMALL_SCENE: c->opt.small_scene = value != 0; c->committed = false; return RTX_OK;
    case RTX_OPT_SMALL_SLABS: c->opt.small_slabs = value != 0; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_FUSED_BOUNCE: c->opt.fused = value != 0; return RTX_OK;
    case RTX_OPT_BOUNCE_VARIANT: c->opt.bounce_variant = value == 2 ? 2 : (value != 0 ? 1 : 0); return RTX_OK;     // 0: workgroup-wide LDS hit ring between trace and shading; 1: trace and shade the same 256 entries; 2: wave-private rings, no barrier inside a bounce
    case RTX_OPT_SHARED_PRIMARY: c->opt.shared_primary = value != 0; return RTX_OK;
    case RTX_OPT_STACK_PRIVATE: c->opt.stack_private = (int)value; c->committed = false; return RTX_OK;
    case RTX_OPT_LPT_ORDER: c->opt.lpt_order = value != 0; return RTX_OK;
    case RTX_OPT_FUSED_BVH: c->opt.fused_bvh = value != 0; return RTX_OK;
    case RTX_OPT_WORK_STEALING: c->opt.work_stealing = value != 0; return RTX_OK;
    case RTX_OPT_COMPACT_STATE: c->opt.compact_state = value != 0; return RTX_OK;
    case RTX_OPT_OVERLAP_SHADOW: c->opt.overlap_shadow = value != 0; return RTX_OK;
    case RTX_OPT_BLOCKS_PER_CU: if (value < 0 || value > 64) { c->err = "blocks_per_cu must be in [0, 64]"; return RTX_ERR_INVALID; } c->opt.blocks_per_cu = (uint32_t)value; return RTX_OK;
    case RTX_OPT_TAPER: if (value < 0 || value > 8) { c->err = "taper must be in [0, 8]"; return RTX_ERR_INVALID; } c->opt.taper = value != 0; c->opt.taper_levels = value == 1 ? 4u : (uint32_t)std::max<long long>(value, 1); return RTX_OK;
    case RTX_OPT_MERGE_RAYS: if (value < 0 || value > (1 << 20)) { c->err = "merge_rays must be in [0, 2^20]"; return RTX_ERR_INVALID; } c->opt.merge_rays = (uint32_t)value; return RTX_OK;
    case RTX_OPT_GPU_REFIT: c->opt.gpu_refit = value != 0; return RTX_OK;
    case RTX_OPT_GPU_BUILD: c->opt.gpu_build = value != 0; return RTX_OK;
    case RTX_OPT_DEFORM_REBUILD: if (value < 0 || value > 1000000) { c->err = "deform_rebuild must be 0 (refit), 1 (rebuild) or a percentage >= 2"; return RTX_ERR_INVALID; } c->opt.deform_rebuild = (int)value; return RTX_OK;
    case RTX_OPT_STACK_CAP: if (value < 0 || value > 30 || (value > 0 && value < 4)) { c->err = "stack_cap must be 0 (the whole stack in LDS) or in [4, 30]"; return RTX_ERR_INVALID; } c->opt.stack_cap = (uint32_t)value; c->committed = false; return RTX_OK;
    case RTX_OPT_SHADE_DENSE: c->opt.shade_dense = (int)value; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_OCCLUDER_CACHE: c->opt.occluder_cache = value != 0; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_RESTIR_WAVEFRONT: c->opt.restir_wave = value != 0; return RTX_OK;
    case RTX_OPT_RESTIR_LANE_MIN: if (value < 256 || value > (1ll << 31)) { c->err = "restir_lane_min must be in [256, 2^31]"; return RTX_ERR_INVALID; } c->opt.restir_lane_min = (uint32_t)value; return RTX_OK;
    case RTX_OPT_RESTIR_LANES: if (value < 1 || value > 4) { c->err = "restir_lanes must be in [1, 4]"; return RTX_ERR_INVALID; } c->opt.restir_lanes = (uint32_t)value; return RTX_OK;
    case RTX_OPT_RESTIR_CHUNKS: if (value < 1 || value > 64) { c->err = "restir_chunks must be in [1, 64]"; return RTX_ERR_INVALID; } c->opt.restir_chunks = (uint32_t)value; return RTX_OK;
    case RTX_OPT_TRACE_SCHED: if (value > 7) { c->err = "trace_sched must be in [0, 7]"; return RTX_ERR_INVALID; } c->opt.trace_sched = (uint32_t)value; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_REFILL_MIN: if (value < 1 || value > 64) { c->err = "refill_min must be in [1, 64]"; return RTX_ERR_INVALID; } c->opt.refill_min = (uint32_t)value; options_to_scene(c, c->committed); return RTX_OK;
    case RTX_OPT_DENOISE_LDS_STEP: if (value != 0 && value != 1 && value != 2 && value != 4) { c->err = "denoise_lds_step must be 0, 1, 2 or 4"; return RTX_ERR_INVALID; } c->dn.lds_step = (uint32_t)value; return RTX_OK;
    default: c->err = "unknown option"; return RTX_ERR_INVALID;
    }
}

int rtx_set_stream(rtx_ctx* c, void* s) {
    BIND(c);
    if (c->own_stream && c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    else HIPCHK(c, hipDeviceSynchronize());                // the old caller-owned stream may no longer exist: drain the device instead of touching it
    if (c->own_stream) { c->stream = nullptr; c->own_stream = false; }
    if (s) { c->stream = (hipStream_t)s; c->own_stream = false; }
    else { c->stream = c->streams.set.s[0]; c->own_stream = true; }
    return RTX_OK;
}

int rtx_set_materials(rtx_ctx* c, const void* mats128, uint32_t count) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.set_materials(mats128, count)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_add_mesh(rtx_ctx* c, const void* verts28, uint32_t nverts, const uint32_t* indices, uint32_t nidx, const uint32_t* material_ids, uint32_t* mesh_out) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.add_mesh(verts28, nverts, indices, nidx, material_ids, mesh_out)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_add_instance(rtx_ctx* c, uint32_t mesh, const float o2w[16], uint32_t* inst_out) {
    if (!c || !o2w) return RTX_ERR_INVALID;
    if (!c->host.add_instance(mesh, o2w, inst_out)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_set_instance_transform(rtx_ctx* c, uint32_t inst, const float o2w[16]) {
    if (!c || !o2w) return RTX_ERR_INVALID;
    if (!c->host.set_instance_transform(inst, o2w)) { c->err = c->host.err; return RTX_ERR_INVALID; }
    c->committed = false; return RTX_OK;
}
int rtx_set_instance_visible(rtx_ctx* c, uint32_t inst, int visible) {
    if (!c) return RTX_ERR_INVALID;
    bool changed = false;
    if (!c->host.set_instance_visible(inst, visible != 0, &changed)) { c->err = c->host.err; return RTX_ERR_INVALID; }     // (nothing changed: the scene stays committed)
    if (changed) c->committed = false;                     // the value it already had: nothing to commit
    return RTX_OK;
}

int rtx_update_mesh_vertices(rtx_ctx* c, uint32_t mesh, const void* verts28, uint32_t nverts) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->host.update_mesh_vertices(mesh, verts28, nverts)) { c->err = c->host.err; return RTX_ERR_INVALID; }     // (nothing changed: the scene stays committed)
    c->committed = false; return RTX_OK;
}

int rtx_set_camera(rtx_ctx* c, const float view[16], const float proj[16]) {
    BIND(c);
    if (!view || !proj) return RTX_ERR_INVALID;
    // previous-frame matrices for the temporal pass (m_prevViewMatrix / m_prevProjMatrix, Renderer.cpp:1738-1740, 1766-1767)
    if (c->camera_set) { memcpy(c->prev_view, c->view, 64); memcpy(c->prev_proj, c->proj, 64); }
    else { memcpy(c->prev_view, view, 64); memcpy(c->prev_proj, proj, 64); }
    memcpy(c->view, view, 64); memcpy(c->proj, proj, 64);
    CameraGPU cam;
    mat4_inverse(view, cam.viewI); mat4_inverse(proj, cam.projI);     // Renderer.cpp:1735-1736
    memcpy(cam.prev_view, c->prev_view, 64); memcpy(cam.prev_proj, c->prev_proj, 64);
    HIPCHK(c, c->d_cam.ensure(sizeof(cam)));
    TO_DEVICE(c, c->d_cam.p, &cam, sizeof(cam));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->camera_set = true;
    return RTX_OK;
}

// camera state like the matrices: no commit, nothing of the scene is touched; every later frame of rtx_render / rtx_render_adaptive reads it through make_frame
int rtx_set_lens(rtx_ctx* c, const rtx_lens* lens) {
    BIND(c);
    if (!lens) { c->lens = rtx_lens{}; return RTX_OK; }
    const float R = lens->aperture_radius, F = lens->focus_distance;
    if (!std::isfinite(R) || R < 0.0f) { c->err = "set_lens: aperture_radius must be finite and >= 0"; return RTX_ERR_INVALID; }
    if (!std::isfinite(F) || (R > 0.0f && !(F > 0.0f))) { c->err = "set_lens: focus_distance must be finite, and > 0 with an open aperture"; return RTX_ERR_INVALID; }
    if (lens->reserved[0] || lens->reserved[1]) { c->err = "set_lens: reserved words must be 0"; return RTX_ERR_INVALID; }
    c->lens = *lens;
    return RTX_OK;
}
// autofocus: the view-axis depth of what pixel (x, y)'s pinhole ray sees first (k_focus_distance: the ray and trace of the debug layers)
int rtx_focus_distance_at(rtx_ctx* c, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float* distance_out) {
    BIND(c);
    if (!c->committed || !c->camera_set) { c->err = "focus_distance_at: scene not committed or camera not set"; return RTX_ERR_STATE; }
    if (!distance_out || !width || !height || x >= width || y >= height) { c->err = "focus_distance_at: pixel outside the image"; return RTX_ERR_INVALID; }
    DevBuf d_out;
    HIPCHK(c, d_out.ensure(4));
    launch_focus_distance(c->stream, c->dsc, width, height, (const CameraGPU*)c->d_cam.p, x, y, (float*)d_out.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, distance_out, d_out.p, 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_bind_accum(rtx_ctx* c, void* dev, size_t bytes) {
    if (!c) return RTX_ERR_INVALID;
    c->ext_accum = dev; c->ext_accum_bytes = dev ? bytes : 0;
    return RTX_OK;
}

int rtx_clear_accum(rtx_ctx* c, uint32_t w, uint32_t h) {
    BIND(c);
    if (!w || !h) return RTX_ERR_INVALID;
    int r = ensure_accum(c, w, h, true);
    if (r) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}


int rtx_read_accum(rtx_ctx* c, float* out, size_t bytes) {
    BIND(c);
    const size_t need = (size_t)c->acc_w * c->acc_h * 16;
    if (!out || !need || bytes < need || !c->accum_ptr()) { c->err = "read_accum: no image or buffer too small"; return RTX_ERR_INVALID; }
    TO_HOST(c, out, c->accum_ptr(), need);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_read_srgb8(rtx_ctx* c, uint8_t* out, size_t bytes) {
    BIND(c);
    const uint32_t npix = c->acc_w * c->acc_h;
    if (!out || !npix || bytes < (size_t)npix * 4 || !c->accum_ptr()) { c->err = "read_srgb8: no image or buffer too small"; return RTX_ERR_INVALID; }
    HIPCHK(c, c->d_srgb.ensure((size_t)npix * 4));
    launch_srgb8(c->stream, c->accum_ptr(), npix, (uint32_t*)c->d_srgb.p);
    TO_HOST(c, out, c->d_srgb.p, (size_t)npix * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

// gOutput layer `layer` of the reference's 30-layer output array (Renderer.h:298-299): 0 = the image (== rtx_read_srgb8); 10-17 = first-hit debug
// attributes (k_debug_layer); every other layer below 30 reads black, as in the reference whose shaders never write them
int rtx_read_layer(rtx_ctx* c, uint32_t layer, uint32_t width, uint32_t height, uint8_t* out, size_t bytes) {
    BIND(c);
    if (layer >= 30u) { c->err = "read_layer: the output array has 30 layers"; return RTX_ERR_INVALID; }
    if (layer == 0u) { if (width != c->acc_w || height != c->acc_h) { c->err = "read_layer: layer 0 has the size of the accumulation buffer"; return RTX_ERR_INVALID; } return rtx_read_srgb8(c, out, bytes); }
    const size_t npix = (size_t)width * height;
    if (!out || !npix || npix > 0x7FFFFFFFull || bytes < npix * 4) { c->err = "read_layer: bad size"; return RTX_ERR_INVALID; }
    if (layer < 10u || layer > 17u) { memset(out, 0, npix * 4); for (size_t i = 0; i < npix; i++) out[i * 4 + 3] = 255; return RTX_OK; }
    if (!c->committed || !c->camera_set) { c->err = "read_layer: scene not committed or camera not set"; return RTX_ERR_STATE; }
    HIPCHK(c, c->d_srgb.ensure(npix * 4));
    launch_debug_layer(c->stream, (uint32_t)c->num_cus * 8u, c->dsc, width, height, (const CameraGPU*)c->d_cam.p, layer, (uint32_t*)c->d_srgb.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out, c->d_srgb.p, npix * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_get_stats(rtx_ctx* c, rtx_stats* out) { if (!out) return RTX_ERR_INVALID; BIND(c); *out = c->stats; return RTX_OK; }     // (joins a frame that RTX_OPT_ASYNC left in flight)

int rtx_get_lights(rtx_ctx* c, void* out80, uint32_t max_count, uint32_t* count_out) {
    if (!c) return RTX_ERR_INVALID;
    if (!c->committed) { c->err = "get_lights: scene not committed"; return RTX_ERR_STATE; }
    const uint32_t n = (uint32_t)(c->scene.built.lights80.size() / 20);
    if (count_out) *count_out = n;
    if (out80) memcpy(out80, c->scene.built.lights80.data(), (size_t)std::min(n, max_count) * 80);
    return RTX_OK;
}

int rtx_shard_slab_bytes(const rtx_params* p, size_t* bytes) {
    if (!bytes) return RTX_ERR_INVALID;
    uint32_t ts = 0, cnt = 0; uint64_t npl = 0;
    if (const char* e = validate_tiling(p, ts, cnt, npl)) { g_create_err = e; return RTX_ERR_INVALID; }   // no context here: message via rtx_last_error(NULL)
    *bytes = (size_t)npl * 16;
    return RTX_OK;
}
int rtx_pack_tiles(rtx_ctx* c, const rtx_params* p, void* slab) {
    BIND_NOWAIT(c);                       // stream-ordered behind an enqueued rtx_render (RTX_OPT_ASYNC): no host join
    DevFrame f; int r = make_frame(c, p, f); if (r) return r;
    if (!slab || !c->accum_ptr() || c->acc_w != p->width || c->acc_h != p->height) { c->err = "pack_tiles: no accumulation buffer of that size"; return RTX_ERR_STATE; }
    launch_pack_tiles(c->stream, (uint32_t)c->num_cus * 8u, f, c->accum_ptr(), (F4*)slab);
    HIPCHK(c, hipGetLastError());
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));     // on a caller-bound stream the gather that follows is stream-ordered: no host bubble
    return RTX_OK;
}
int rtx_unpack_tiles(rtx_ctx* c, const rtx_params* p, const void* slabs) {
    BIND_NOWAIT(c);                       // stream-ordered behind an enqueued rtx_render (RTX_OPT_ASYNC): no host join
    DevFrame f; int r = make_frame(c, p, f); if (r) return r;
    if (!slabs) return RTX_ERR_INVALID;
    if ((r = ensure_accum(c, p->width, p->height, false))) return r;
    c->ad.whole = false;                  // u1 gets samples `half` does not hold (gathering `half` is not offered)
    launch_unpack_tiles(c->stream, (uint32_t)c->num_cus * 8u, f, f.shard_count, (const F4*)slabs, c->accum_ptr());
    HIPCHK(c, hipGetLastError());
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"

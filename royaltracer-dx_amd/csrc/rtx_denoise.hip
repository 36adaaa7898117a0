// rtx_denoise.hip — rtx_denoise and rtx_denoise_variance: the edge-avoiding a-trous filters over the mean of u1, and the reads of the denoised image.  Validate, guides
// (k_denoise_guides, one primary ray per pixel, every call; with a flag of the parameters set the form that writes the map-guide record too), then one k_denoise_level per level
// between u1, two ping-pong images and the denoised image.  Part of the C-ABI of include/rtx.h (rtx_ctx.hpp); the kernels and the tap arithmetic: rtx_k_denoise.hpp.
// rtx_denoise_variance is the same sequence with the level kernel's VAR forms: they read `half`, the adaptive sampler's second sum, beside u1 (half_state: when that sum belongs
// to u1); rtx_read_adaptive_half and rtx_debug_denoise_variance show its two inputs.
#include <cmath>
#include "rtx_ctx.hpp"

// the default sigma_plane's box, by the float32 operations include/rtx.h names (this file is compiled without contraction): every vertex of every instance's mesh
static float scene_largest_extent(const SceneHost& H) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const InstHost& in : H.insts) {
        const std::vector<float>& v = H.meshes[in.mesh].verts; const float* m = in.o2w;
        for (size_t i = 0; i + 7 <= v.size(); i += 7)
            for (int k = 0; k < 3; k++) {
                const float w = ((v[i] * m[k] + v[i + 1] * m[4 + k]) + v[i + 2] * m[8 + k]) + m[12 + k];
                lo[k] = w < lo[k] ? w : lo[k]; hi[k] = w > hi[k] ? w : hi[k];
            }
    }
    const float e[3] = {hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]};
    return std::max(e[0], std::max(e[1], e[2]));
}

// a denoised image of the accumulation buffer's size exists
static bool have_denoised(rtx_ctx* c) { return c->dn.valid && c->dn.d_out.p && c->dn.w == c->acc_w && c->dn.h == c->acc_h; }

// what the two filters check alike (their parameter structs differ in the meaning of one float): state, size, flags, reserved words, levels and power; q = *dp with the
// defaults of levels and normal_power_log2 filled in
template <class P> static int filter_checks(rtx_ctx* c, const char* who, uint32_t width, uint32_t height, const P* dp, P& q) {
    const std::string w = std::string(who) + ": ";
    if (!c->committed) { c->err = w + "scene not committed"; return RTX_ERR_STATE; }
    if (!c->camera_set) { c->err = w + "camera not set"; return RTX_ERR_STATE; }
    if (!c->accum_ptr() || !c->acc_w || !c->acc_h) { c->err = w + "no accumulation buffer yet"; return RTX_ERR_STATE; }
    if (width != c->acc_w || height != c->acc_h) { c->err = w + "the size differs from the accumulation buffer's"; return RTX_ERR_INVALID; }
    const size_t npix = (size_t)width * height;
    if (npix > 0x7FFFFFFFull) { c->err = w + "image too large"; return RTX_ERR_INVALID; }
    if (c->ext_accum && c->ext_accum_bytes < npix * 16) { c->err = "bound accumulation buffer is smaller than width*height*16 bytes"; return RTX_ERR_INVALID; }
    if (dp) q = *dp;
    if (q.flags & ~(RTX_DENOISE_ALBEDO | RTX_DENOISE_MAPPED_NORMALS)) { c->err = w + "unknown bits in flags"; return RTX_ERR_INVALID; }
    for (uint32_t r : q.reserved) if (r) { c->err = w + "reserved words must be 0"; return RTX_ERR_INVALID; }
    if (q.levels > 8 || q.normal_power_log2 > 7) { c->err = w + "levels must be in [1, 8] and normal_power_log2 in [1, 7] (0 = default)"; return RTX_ERR_INVALID; }
    if (!q.levels) q.levels = 5;
    if (!q.normal_power_log2) q.normal_power_log2 = 5;
    return RTX_OK;
}

// what rtx_denoise and rtx_denoise_variance share once their arguments are validated: memory, guides, the levels, the result.  variance: the levels are the VAR forms of
// k_denoise_level, which read `half` beside u1 at level 0 and take sigma = sigma_var; else the plain forms with sigma = 1 / sigma_color
static int filter_levels(rtx_ctx* c, uint32_t width, uint32_t height, uint32_t levels, uint32_t normal_power_log2, float inv_plane, uint32_t flags, bool variance, float sigma, rtx_denoise_result* out) {
    const size_t npix = (size_t)width * height;
    // ---- 2. memory: allocated on first use, resized with the image ----
    rtx_ctx::Denoise& D = c->dn;
    const uint32_t nwg = denoise_workgroups(width, height);
    HIPCHK(c, D.d_guides.ensure(npix * 32)); if (flags) HIPCHK(c, D.d_mguides.ensure(npix * 32));
    HIPCHK(c, D.d_partial.ensure((size_t)nwg * 4)); HIPCHK(c, D.d_count.ensure(16));
    if (levels > 1) HIPCHK(c, D.d_pp[0].ensure(npix * 16));
    if (levels > 2) HIPCHK(c, D.d_pp[1].ensure(npix * 16));
    HIPCHK(c, D.d_out.ensure(npix * 16));
    D.valid = false; D.w = width; D.h = height;

    // ---- 3. guides, then the levels: u1 (and `half`) -> pp[0] -> pp[1] -> ... -> the denoised image ----
    const hipStream_t st = c->stream;
    const bool timing = c->opt.timing;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    D.ev.used = 0;
    if (timing) for (hipEvent_t& e : ev) e = D.ev.take();
    const bool timed = timing && ev[0] && ev[1] && ev[2] && ev[3];
    if (timed) (void)hipEventRecord(ev[0], st);
    F4* mg = flags ? (F4*)D.d_mguides.p : nullptr;                      // (the buffer may outlive a call with a flag set: this call's flags decide, not its pointer)
    launch_denoise_guides(st, (uint32_t)c->num_cus * 8u, c->dsc, width, height, (const CameraGPU*)c->d_cam.p, (F4*)D.d_guides.p, mg);
    if (timed) { (void)hipEventRecord(ev[1], st); (void)hipEventRecord(ev[2], st); }
    const F4* in = c->accum_ptr();
    for (uint32_t i = 0; i < levels; i++) {
        DenoiseLevel a{};
        a.width = width; a.height = height; a.step = 1u << i; a.normal_power_log2 = normal_power_log2; a.first = i == 0; a.last = i + 1 == levels;
        a.inv_sigma_plane = inv_plane; a.inv_sigma_color_s = variance ? 0.0f : sigma * (float)a.step;
        F4* dst = (F4*)(a.last ? D.d_out.p : D.d_pp[i & 1u].p);
        launch_denoise_level(st, a, variance, variance ? sigma : 0.0f, flags, in, variance ? (const F4*)c->ad.d_half.p : nullptr, (const F4*)D.d_guides.p, mg, dst, (uint32_t*)D.d_partial.p, a.step <= D.lds_step);
        in = dst;
    }
    if (timed) (void)hipEventRecord(ev[3], st);
    if (out) launch_denoise_count(st, (const uint32_t*)D.d_partial.p, nwg, (uint32_t*)D.d_count.p);
    HIPCHK(c, hipGetLastError());
    D.valid = true;
    if (out) {
        uint32_t filtered = 0;
        TO_HOST(c, &filtered, D.d_count.p, 4);                               // (complete when it returns: the stream is joined up to here)
        *out = rtx_denoise_result{};
        out->levels = levels; out->pixels_filtered = filtered; out->pixels_passed = (uint32_t)npix - filtered;
        if (timed) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, ev[0], ev[1]) == hipSuccess) out->guides_ms = ms;
            if (hipEventElapsedTime(&ms, ev[2], ev[3]) == hipSuccess) out->filter_ms = ms;
        }
    }
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));            // on a caller-bound stream what follows is stream-ordered: no host bubble
    return RTX_OK;
}

// what the rtx_debug_denoise_* entry points share: the state check, check(npix) — the entry point's own checks, RTX_OK to go on —, PRIVATE records (a debug call must not
// disturb the filter's own, nor a denoised image of another size), the guides launch (maps: the form that writes the map-guide record too) and the copy back.  out_item = 0:
// `out` receives the record itself (the map-guide record when maps), 32 bytes per pixel; else second(guides, mguides, d_out) launches the kernel that writes out_item bytes per pixel
template <class Check, class Second>
static int guides_probe(rtx_ctx* c, const char* name, uint32_t width, uint32_t height, bool maps, void* out, size_t out_item, Check check, Second second) {
    BIND(c);
    if (!c->committed || !c->camera_set) { c->err = std::string(name) + ": scene not committed or camera not set"; return RTX_ERR_STATE; }
    const size_t npix = (size_t)width * height;
    if (const int r = check(npix)) return r;
    DevBuf d_g, d_m, d_o;
    HIPCHK(c, d_g.ensure(npix * 32));
    if (maps) HIPCHK(c, d_m.ensure(npix * 32));
    if (out_item) HIPCHK(c, d_o.ensure(npix * out_item));
    launch_denoise_guides(c->stream, (uint32_t)c->num_cus * 8u, c->dsc, width, height, (const CameraGPU*)c->d_cam.p, (F4*)d_g.p, (F4*)d_m.p);
    if (out_item) second((const F4*)d_g.p, (const F4*)d_m.p, d_o.p);
    HIPCHK(c, hipGetLastError());
    TO_HOST(c, out, out_item ? d_o.p : (maps ? d_m.p : d_g.p), npix * (out_item ? out_item : 32));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}
// the two entry points that return a record
static int record_probe(rtx_ctx* c, const char* name, uint32_t width, uint32_t height, bool maps, float* out8) {
    return guides_probe(c, name, width, height, maps, out8, 0, [&](size_t npix) {
        if (!out8 || !npix || npix > 0x7FFFFFFFull) { c->err = std::string(name) + ": bad size"; return RTX_ERR_INVALID; }
        return RTX_OK;
    }, [](const F4*, const F4*, void*) {});
}

extern "C" {

int rtx_denoise(rtx_ctx* c, uint32_t width, uint32_t height, const rtx_denoise_params* dp, rtx_denoise_result* out) {
    // ---- 1. validate: a call that fails leaves u1 and the previous denoised image untouched ----
    BIND_NOWAIT(c);                       // stream-ordered behind an enqueued rtx_render (RTX_OPT_ASYNC): no host join
    rtx_denoise_params q{};
    if (const int r = filter_checks(c, "denoise", width, height, dp, q)) return r;
    if (!(q.sigma_color >= 0.0f) || !(q.sigma_plane >= 0.0f) || std::isinf(q.sigma_color) || std::isinf(q.sigma_plane)) { c->err = "denoise: sigma_color and sigma_plane must be finite and > 0 (0 = default)"; return RTX_ERR_INVALID; }
    if (q.sigma_color == 0.0f) q.sigma_color = 0.5f;
    if (q.sigma_plane == 0.0f) q.sigma_plane = 0.015625f * scene_largest_extent(c->host);
    const float inv_color = 1.0f / q.sigma_color, inv_plane = 1.0f / q.sigma_plane;
    if (!std::isfinite(inv_color) || !std::isfinite(inv_plane) || !std::isfinite(inv_color * (float)(1u << (q.levels - 1u)))) { c->err = "denoise: a sigma is too small (or the scene has no extent for the default sigma_plane)"; return RTX_ERR_INVALID; }
    return filter_levels(c, width, height, q.levels, q.normal_power_log2, inv_plane, q.flags, false, inv_color, out);
}

// the adaptive state that belongs to u1 (rtx.h, VARIANCE-GUIDED, STATE): null, or why `half` is not the second sum of every pixel of a width x height u1
static const char* half_state(rtx_ctx* c, uint32_t width, uint32_t height) {
    const rtx_ctx::Adaptive& A = c->ad;
    if (!A.pure) return "the image holds samples of rtx_render / rtx_render_v6_pass1 / rtx_render_restir";
    if (A.cleared || !A.d_half.p) return "no rtx_render_adaptive since the image was cleared";
    if (A.key[0] != width || A.key[1] != height) return "the adaptive state is laid out for another size";
    if (!A.whole) return "the image was sampled on shards (rtx_render_adaptive with shard_count > 1, or rtx_unpack_tiles)";
    return nullptr;
}

int rtx_denoise_variance(rtx_ctx* c, uint32_t width, uint32_t height, const rtx_denoise_var_params* dp, rtx_denoise_result* out) {
    // ---- 1. validate, as rtx_denoise does: a call that fails leaves u1, `half` and the previous denoised image untouched ----
    BIND_NOWAIT(c);
    rtx_denoise_var_params q{};
    if (const int r = filter_checks(c, "denoise_variance", width, height, dp, q)) return r;
    if (!(q.sigma_var >= 0.0f) || !(q.sigma_plane >= 0.0f) || std::isinf(q.sigma_var) || std::isinf(q.sigma_plane)) { c->err = "denoise_variance: sigma_var and sigma_plane must be finite and > 0 (0 = default)"; return RTX_ERR_INVALID; }
    if (q.sigma_var == 0.0f) q.sigma_var = 4.0f;
    if (q.sigma_plane == 0.0f) q.sigma_plane = 0.015625f * scene_largest_extent(c->host);
    const float inv_plane = 1.0f / q.sigma_plane;
    if (!std::isfinite(1.0f / q.sigma_var) || !std::isfinite(inv_plane)) { c->err = "denoise_variance: a sigma is too small (or the scene has no extent for the default sigma_plane)"; return RTX_ERR_INVALID; }
    if (const char* why = half_state(c, width, height)) { c->err = std::string("denoise_variance: ") + why + "; rtx_clear_accum, then rtx_render_adaptive"; return RTX_ERR_STATE; }

    return filter_levels(c, width, height, q.levels, q.normal_power_log2, inv_plane, q.flags, true, q.sigma_var, out);
}

int rtx_read_adaptive_half(rtx_ctx* c, float* out, size_t bytes) {
    BIND(c);
    if (!c->accum_ptr() || !c->acc_w || !c->acc_h) { c->err = "read_adaptive_half: no accumulation buffer yet"; return RTX_ERR_STATE; }
    if (const char* why = half_state(c, c->acc_w, c->acc_h)) { c->err = std::string("read_adaptive_half: ") + why; return RTX_ERR_STATE; }
    const size_t need = (size_t)c->acc_w * c->acc_h * 16;
    if (!out || bytes < need) { c->err = "read_adaptive_half: buffer too small"; return RTX_ERR_INVALID; }
    TO_HOST(c, out, c->ad.d_half.p, need);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_debug_denoise_variance(rtx_ctx* c, uint32_t width, uint32_t height, uint32_t flags, float* out2) {
    const bool alb = (flags & RTX_DENOISE_ALBEDO) != 0;                        // (the normals of the normal stop do not enter v or gv)
    return guides_probe(c, "denoise_variance_input", width, height, alb, out2, 8, [&](size_t npix) {
        if (!c->accum_ptr() || !c->acc_w || !c->acc_h) { c->err = "denoise_variance_input: no accumulation buffer yet"; return RTX_ERR_STATE; }
        if (!out2 || width != c->acc_w || height != c->acc_h || npix > 0x7FFFFFFFull || (flags & ~(RTX_DENOISE_ALBEDO | RTX_DENOISE_MAPPED_NORMALS))) { c->err = "denoise_variance_input: bad size or flags"; return RTX_ERR_INVALID; }
        if (c->ext_accum && c->ext_accum_bytes < npix * 16) { c->err = "bound accumulation buffer is smaller than width*height*16 bytes"; return RTX_ERR_INVALID; }
        if (const char* why = half_state(c, width, height)) { c->err = std::string("denoise_variance_input: ") + why; return RTX_ERR_STATE; }
        return RTX_OK;
    }, [&](const F4* guides, const F4* mguides, void* out) { launch_denoise_var_input(c->stream, width, height, alb, c->accum_ptr(), (const F4*)c->ad.d_half.p, guides, mguides, (float*)out); });
}

int rtx_read_denoised(rtx_ctx* c, float* out, size_t bytes) {
    BIND(c);
    if (!have_denoised(c)) { c->err = "read_denoised: no denoised image of the accumulation buffer's size (rtx_denoise first)"; return RTX_ERR_STATE; }
    const size_t need = (size_t)c->dn.w * c->dn.h * 16;
    if (!out || bytes < need) { c->err = "read_denoised: buffer too small"; return RTX_ERR_INVALID; }
    TO_HOST(c, out, c->dn.d_out.p, need);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_read_denoised_srgb8(rtx_ctx* c, uint8_t* out, size_t bytes) {
    BIND(c);
    if (!have_denoised(c)) { c->err = "read_denoised_srgb8: no denoised image of the accumulation buffer's size (rtx_denoise first)"; return RTX_ERR_STATE; }
    const uint32_t npix = c->dn.w * c->dn.h;
    if (!out || bytes < (size_t)npix * 4) { c->err = "read_denoised_srgb8: buffer too small"; return RTX_ERR_INVALID; }
    HIPCHK(c, c->d_srgb.ensure((size_t)npix * 4));
    launch_srgb8(c->stream, (const F4*)c->dn.d_out.p, npix, (uint32_t*)c->d_srgb.p);
    TO_HOST(c, out, c->d_srgb.p, (size_t)npix * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_debug_denoise_guides(rtx_ctx* c, uint32_t width, uint32_t height, float* out8) { return record_probe(c, "denoise_guides", width, height, false, out8); }
int rtx_debug_denoise_map_guides(rtx_ctx* c, uint32_t width, uint32_t height, float* out8) { return record_probe(c, "denoise_map_guides", width, height, true, out8); }

}  // extern "C"

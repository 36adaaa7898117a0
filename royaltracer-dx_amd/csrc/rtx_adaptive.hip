// rtx_adaptive.hip — rtx_render_adaptive: the path tracer's frame sampled until its 256-slot chunks have converged.  Validate, then repeat: the criterion per chunk
// (k_adaptive_error), the active list (k_adaptive_compact), its length read back, one pass of render_frame (rtx_render.hip) over the list.  Part of the C-ABI of
// include/rtx.h (rtx_ctx.hpp); the kernels and the criterion: rtx_k_adaptive.hpp.
#include "rtx_ctx.hpp"

extern "C" {

int rtx_render_adaptive(rtx_ctx* c, const rtx_params* p, const rtx_adaptive* a, rtx_adaptive_result* out) {
    // ---- 1. validate: a call that fails leaves image and state untouched ----
    DevFrame f;
    int r = render_checks(c, p, false, f);
    if (r) return r;
    if (!a) { c->err = "render_adaptive: no rtx_adaptive"; return RTX_ERR_INVALID; }
    // the two half sums are equally large only at even counts
    if (a->min_spp < 2 || (a->min_spp & 1u) || a->step_spp < 2 || (a->step_spp & 1u)) { c->err = "render_adaptive: min_spp and step_spp must be even and >= 2"; return RTX_ERR_INVALID; }
    if (a->min_spp > a->max_spp) { c->err = "render_adaptive: min_spp > max_spp"; return RTX_ERR_INVALID; }
    if (!(a->threshold >= 0.0f) || !(a->dark_floor >= 0.0f) || a->threshold > 3.0e38f || a->dark_floor > 3.0e38f) { c->err = "render_adaptive: threshold and dark_floor must be finite and >= 0"; return RTX_ERR_INVALID; }
    if ((uint64_t)p->sample_base + a->max_spp > 0xFFFFFFFFull) { c->err = "render_adaptive: sample_base + max_spp overflows"; return RTX_ERR_INVALID; }
    if (!c->ad.pure) { c->err = "render_adaptive: the image holds samples of rtx_render / rtx_render_v6_pass1 / rtx_render_restir; rtx_clear_accum first"; return RTX_ERR_STATE; }
    const bool had_image = c->ext_accum || (c->d_accum.p && c->acc_w == p->width && c->acc_h == p->height);
    const uint32_t key[3] = {p->width, p->height, f.tile_size};
    if (had_image && !c->ad.cleared && memcmp(key, c->ad.key, sizeof(key)) != 0) { c->err = "render_adaptive: the image was sampled with another size or tile_size; rtx_clear_accum first"; return RTX_ERR_STATE; }
    if ((r = ensure_accum(c, p->width, p->height, false))) return r;          // (a fresh image is a cleared one)

    // ---- 2. the state: zeroed by the first call after a clear ----
    const size_t npix = (size_t)p->width * p->height, nwords = ((size_t)f.tiles_x * f.tiles_y) << (2u * f.tile_shift - 8u);
    HIPCHK(c, c->ad.d_half.ensure(npix * 16)); HIPCHK(c, c->ad.d_count.ensure(nwords * 4)); HIPCHK(c, c->ad.d_flag.ensure(nwords * 4));
    HIPCHK(c, c->ad.d_list.ensure((size_t)f.chunks_per_sample * 4)); HIPCHK(c, c->ad.d_out.ensure(32));
    const hipStream_t st = c->stream;
    if (c->ad.cleared) {
        HIPCHK(c, hipMemsetAsync(c->ad.d_half.p, 0, npix * 16, st)); HIPCHK(c, hipMemsetAsync(c->ad.d_count.p, 0, nwords * 4, st)); HIPCHK(c, hipMemsetAsync(c->ad.d_flag.p, 0, nwords * 4, st));
        c->ad.cleared = false; memcpy(c->ad.key, key, sizeof(key)); c->ad.whole = true;
    }
    if (p->shard_count > 1) c->ad.whole = false;                             // (`half` of the other shards' pixels stays zero: rtx_denoise_variance refuses)
    const AdaptState S{(F4*)c->ad.d_half.p, (uint32_t*)c->ad.d_count.p, (uint32_t*)c->ad.d_flag.p};
    uint32_t* list = (uint32_t*)c->ad.d_list.p;
    const float dark_floor = a->dark_floor == 0.0f ? 0.01f : a->dark_floor;
    stats_begin(c);

    // ---- 3. the passes.  Synchronous whatever RTX_OPT_ASYNC says: the host sizes every pass by the list's length ----
    uint32_t h[5] = {0, 0, 0, 0, 0}, passes = 0;
    uint64_t evaluated = 0;
    for (;;) {
        { Timed t(c, RTX_K_ADAPT); launch_adaptive_error(st, f, c->accum_ptr(), S, a->threshold, dark_floor); }
        { Timed t(c, RTX_K_ADAPT); launch_adaptive_compact(st, f, S, a->max_spp, list, (uint32_t*)c->ad.d_out.p); }
        HIPCHK(c, hipGetLastError());
        TO_HOST(c, h, c->ad.d_out.p, sizeof(h));                             // (complete when it returns)
        collect_timed(c);
        evaluated += f.chunks_per_sample;
        if (!h[0]) break;                                                    // every chunk has converged or is at max_spp
        // all chunks of the list hold h[1] samples: none yet -> min_spp; else step_spp more, or fewer to land on max_spp
        const uint32_t cur = h[1], step = cur < a->min_spp ? a->min_spp - cur : std::min(a->step_spp, a->max_spp - cur);
        const ListPass lp{list, h[0], p->sample_base + cur, S, passes == 0};
        if ((r = render_frame(c, p, f, step, &lp))) return r;
        if ((r = finish_render(c))) return r;
        passes++;
    }
    c->stats.kernel_items[RTX_K_ADAPT] = evaluated;
    if (out) { out->passes = passes; out->chunks = h[4]; out->chunks_converged = h[2]; out->chunks_at_max = h[3]; out->pixel_samples = c->stats.paths; }
    return RTX_OK;
}

}  // extern "C"

// rtx_render.hip — rtx_render, the wavefront path tracer's frame: validate, then (render_frame, shared with the passes of rtx_render_adaptive) plan the batches, size the
// buffers, enqueue every batch by one of three schedules (the fused tiny-scene kernels, one k_bounce_bvh launch, or the separate trace / shade / shadow kernels per bounce),
// and collect the counters (finish_render).  Part of the C-ABI of include/rtx.h (rtx_ctx.hpp).
#include "rtx_ctx.hpp"

namespace {

// the layout of a frame's batches: samples per batch, G workgroups (each with a private sub-queue: no global atomics in the loop), the longest sub-queue in 256-path chunks,
// taper levels, the workgroup count of the grid-wide launches, and whether the path state lives by queue position (compact)
struct BatchPlan { uint32_t bspp, G, qchunks, taper_levels, max_blocks; bool compact; };

BatchPlan plan_batches(const rtx_ctx* c, uint32_t spp, const DevFrame& f, bool fused_bvh) {
    BatchPlan B{};
    B.bspp = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(spp, c->opt.paths_per_batch / f.npl));
    // sub-queues per CU: shorter tails with more, but more per-workgroup overhead; the fused tiny-scene kernels (5 workgroups resident per
    // CU, longest-first dispatch, all bounces >= 1 in one launch) measured 18.39 / 18.15 / 18.13 / 18.30 / 18.36 ms at 24 / 32 / 40 / 48 / 64
    // (a 1/4 shard: 5.22 / 4.96 / 4.99 / 4.92 / 4.96 ms; 30 is an outlier, its sub-queues alias with the 8100 image regions); the
    // general path: 16 was best in round 1 (49.3 / 42.2 ms vs 53.0 / 44.2 at 8) with 4-6 workgroups resident per CU; with the 7-8 of the end of round 2
    // (LDS trimmed) it is 32: C3 39.8 vs 40.7 ms, C5 37.8 vs 38.2 (48: 40.4 / 39.0)
    // (round 3) ... and never so many that a sub-queue starts with fewer than ~8 (tiny scenes: ~16) chunks of 256 paths while there are 8 workgroups per CU: a 1/8 shard of the
    // 1080p frame (16 200 chunks at 16 spp) ran 7.29 / 6.71 / 6.30 / 6.09 / 6.08 ms with 32 / 24 / 16 / 12 / 8 sub-queues per CU (C3), Cornell at 64 spp 2.54 / 2.41 ms with 40 / 16
    // (tools/shard_kernels.py): short sub-queues leave the persistent waves of a workgroup half empty, and every round of workgroups costs one ray latency
    const bool tiny_fused = c->dsc.nsmall && c->opt.fused;
    auto plan = [&](uint32_t spp_batch) {
        const uint32_t nchunks = f.chunks_per_sample * spp_batch;
        const uint32_t bpc_hi = tiny_fused ? 40u : 32u, per_wg = tiny_fused ? 16u : 8u;
        const uint32_t bpc = c->opt.blocks_per_cu ? c->opt.blocks_per_cu
                                                  : std::max<uint32_t>(8u, std::min<uint32_t>(bpc_hi, (nchunks / per_wg + (uint32_t)c->num_cus - 1u) / (uint32_t)c->num_cus));
        B.max_blocks = (uint32_t)c->num_cus * bpc;
        B.G = std::max<uint32_t>(1, std::min<uint32_t>(nchunks, B.max_blocks));
        // tapered sub-queue sizes (taper_row_width, rtx_kernels.hpp); needs a few chunks in the shortest sub-queue to mean anything.  The fused tiny-scene kernels take their
        // sub-queues longest first anyway (k_order_queues): tapered, that order has something to work with — headline frame 17.18 -> 17.00 ms (same context, option switched)
        B.taper_levels = 0; B.qchunks = (nchunks + B.G - 1) / B.G;
        if (c->opt.taper && !fused_bvh && B.G >= 64u && nchunks >= 4u * B.G) {
            B.taper_levels = c->opt.taper_levels;
            B.qchunks = 0;                                                                 // sub-queue 0 takes part in every row
            for (uint32_t k = 0, row0 = 0; row0 < nchunks; k++) { row0 += taper_row_width(k, B.G, B.taper_levels); B.qchunks++; }
        }
    };
    plan(B.bspp);
    // MEMORY of the taper: every per-queue-position buffer has the uniform stride G * qcap with qcap = the LONGEST sub-queue, so the weights 8 | 4 | 2 | 1 cost
    // 8 / 5.375 = 1.49 x the entries of the even deal (both compact path-state sets, hit records, both queues, nee x 3 shadow streams: ~ +10 GB at the 128 Mi-path cap).
    // Where the path state lives by queue position (the general path: 176 B + 48 B per NEE slot and entry) RTX_OPT_PATHS_PER_BATCH therefore caps the ENTRIES: the batch shrinks
    // until the tapered layout fits it, so a frame that fitted before the taper fits now.  The fused tiny-scene kernels keep 48 B per entry (two sets by queue
    // position) and their batch stays WHOLE, whatever the taper adds: the headline frame is one batch of 132.7 M paths, and a second batch would change the order of the float
    // additions in k_accumulate, hence the image's bits.  Its 196.6 M entries (10 240 sub-queues of 75 chunks) are 18.9 GB of path state (by path id, RTX_OPT_COMPACT_STATE 0:
    // 6.4 GB); a batch at the 128 Mi-path cap has 199.2 M entries, 19.1 GB.
    // The fused tiny-scene path has the by-position layout in bounce 0 and in the wave-scheduled form of bounces >= 1 (RTX_OPT_BOUNCE_VARIANT 2, the default); a frame that
    // runs a block-scheduled form keeps its state by path id throughout.
    B.compact = c->opt.compact_state && !fused_bvh && (!tiny_fused || c->opt.bounce_variant == 2);
    while (B.taper_levels && B.compact && !tiny_fused && B.bspp > 1u && (uint64_t)B.G * B.qchunks * 256u > c->opt.paths_per_batch) {
        const uint32_t next = (uint32_t)std::max<uint64_t>(1, (uint64_t)B.bspp * c->opt.paths_per_batch / ((uint64_t)B.G * B.qchunks * 256u));
        B.bspp = next < B.bspp ? next : B.bspp - 1u;
        plan(B.bspp);
    }
    return B;
}

// what the enqueue steps of a frame share: the path state, the two queues, the per-workgroup counters of one batch — Q(b): queue lengths entering bounce b (b = 0..mb),
// S(b, j): shadow queue lengths, then one row of paths generated (fused raygen + trace); every workgroup stores its own entry, so nothing needs zeroing per batch
struct FrameRun {
    DevPaths P; uint32_t* queue[2]; uint32_t* cnt; const CameraGPU* cam; hipStream_t st;
    const F4* prim_rec;           // RTX_OPT_SHARED_PRIMARY in effect: the per-pixel primary surface records of this call (nullptr: every sample traces its own camera ray)
    uint32_t rec_npl;             // ... and their stream length: the shard's slots (a pass of rtx_render_adaptive renders a shorter, virtual frame: DevFrame::list)
    uint32_t G, mb, nee, nee1; bool compact, osort, stealing; size_t hstride, nheads;
    uint32_t* Q(uint32_t b) const { return cnt + (size_t)b * G; }
    uint32_t* S(uint32_t b, uint32_t j) const { return cnt + ((size_t)(mb + 1) + (size_t)b * nee1 + j) * G; }
};

// tiny scene: trace + shade + shadow fused; bounce 0 (traced by raygen) and then ALL later bounces in one launch each
int enqueue_tiny_fused(rtx_ctx* c, const FrameRun& R, const DevFrame& fb) {
    const hipStream_t st = R.st;
    uint32_t* gen_row = R.cnt + ((size_t)(R.mb + 1) + (size_t)R.mb * R.nee1) * R.G;
    if (R.prim_rec) { Timed t(c, RTX_K_RAYGEN); launch_raygen_shared(st, fb, R.queue[0], R.Q(0), gen_row, (const unsigned long long*)c->pt.d_prim_hits.p, R.rec_npl); }
    else { Timed t(c, RTX_K_RAYGEN); launch_raygen_trace_small(st, c->dsc, fb, R.P, R.cam, R.queue[0], R.Q(0), gen_row, (const unsigned long long*)c->pt.d_pmask.p); }
    // dispatch order of the fused bounce kernels: longest sub-queue first, from the lengths after the primary rays (the later
    // bounces keep the ranking: survivors are a near-constant fraction)
    const uint32_t* order = nullptr;
    if (c->opt.lpt_order && R.G > 1) { launch_order_queues(st, R.Q(0), R.G, (uint32_t*)c->pt.d_order.p); order = (const uint32_t*)c->pt.d_order.p; }
    const PrimIn prim = prim_in(R.prim_rec, R.rec_npl, fb.npl);      // bounce 0 finds sample and slot from the path id (the batch's npl) and the record streams by the REAL slot (rec_npl)
    { Timed t(c, RTX_K_BOUNCE); launch_bounce_small(st, c->dsc, fb, R.P, 0, 1, R.queue[0], R.queue[1], R.Q(0), R.S(0, 0), order, 0, R.prim_rec ? &prim : nullptr); }
    if (R.mb > 1) { Timed t(c, RTX_K_BOUNCE); launch_bounce_small(st, c->dsc, fb, R.P, 1, R.mb, R.queue[0], R.queue[1], R.Q(0), R.S(0, 0), order, c->opt.bounce_variant); }
    return RTX_OK;
}

// general scenes, RTX_OPT_FUSED_BVH: all bounces of every sub-queue in one launch (k_bounce_bvh), sub-queues longest first
int enqueue_fused_bvh(rtx_ctx* c, const FrameRun& R, const DevFrame& fb) {
    const hipStream_t st = R.st;
    { Timed t(c, RTX_K_RAYGEN); launch_raygen(st, fb, R.P, R.cam, R.queue[0], R.Q(0), R.compact); }
    const uint32_t* ord = nullptr;
    if (c->opt.lpt_order && R.G > 1) { launch_order_queues(st, R.Q(0), R.G, (uint32_t*)c->pt.d_order.p); ord = (const uint32_t*)c->pt.d_order.p; }
    Timed t(c, RTX_K_BOUNCE);
    launch_bounce_bvh(st, c->dsc, fb, R.P, 0, R.mb, R.queue[0], R.queue[1], (uint32_t*)c->pt.d_hitq.p, R.Q(0), R.S(0, 0), ord);
    return RTX_OK;
}

// the separate kernels: per bounce k_trace_closest | k_shade | k_trace_shadow per NEE slot, with the shadow overlap, merged thin launches, work stealing and the octant sort
int enqueue_bounces(rtx_ctx* c, const FrameRun& R, const DevFrame& fb) {
    const hipStream_t st = R.st; const DevPaths& P = R.P;
    const uint32_t G = R.G, mb = R.mb, nee = R.nee, nee1 = R.nee1; const bool compact = R.compact, osort = R.osort, stealing = R.stealing;
    { Timed t(c, RTX_K_RAYGEN); launch_raygen(st, fb, P, R.cam, R.queue[0], R.Q(0), compact); }
    if (stealing) HIPCHK(c, hipMemsetAsync(c->pt.d_heads.p, 0, R.nheads * 4, st));          // one cursor block per trace launch of the batch
    // The shadow rays of bounce b and the closest-hit rays of bounce b + 1 both depend on shade(b) only, so k_trace_shadow(b) runs
    // on a second stream beside k_trace_closest(b + 1); shade(b + 1) waits for it (it overwrites the shadow entries, and both touch rad).  The two
    // persistent kernels fill each other's tails and memory stalls: C3 40.8 -> 40.3 ms, C5 38.3 -> 36.9 ms per frame, images unchanged.  Not while
    // kernels are timed (RTX_OPT_KERNEL_TIMING): overlapping launches have no per-kernel time.
    const bool ovl = c->opt.overlap_shadow && !c->opt.timing;
    if (ovl && !c->pt.aux) c->pt.aux = c->streams.set.s[1];
    hipEvent_t ev_shadow_done = nullptr;
    auto Hd = [&](uint32_t b, uint32_t k) { return stealing ? (uint32_t*)c->pt.d_heads.p + ((size_t)b * (1 + nee1) + k) * R.hstride : nullptr; };
    // sub-queues per workgroup of a traversal launch predicted to hold `rays` rays: double while a workgroup would start with fewer than merge_rays and at least one full
    // round of resident workgroups (8 per CU) remains.  Measured in ONE context, option switched between rounds (tools/ab_frame.py same=1): C3 39.45 -> 38.67 / 38.57 /
    // 38.51 ms per frame at 512 / 1024 / 2048, C5 36.77 -> 35.90 / 35.78 / 36.02; going below one round (4 workgroups per CU) changes nothing
    auto merge_for = [&](uint64_t pred_num, bool have) -> uint32_t {
        if (!have || !c->opt.merge_rays || !c->pt.pred_paths || stealing) return 1u;
        const double rays = (double)pred_num * (double)((uint64_t)fb.npl * fb.batch_spp) / (double)c->pt.pred_paths;
        uint32_t k = 1u;
        while (k < kMaxMerge && G / (2u * k) >= (uint32_t)c->num_cus * 8u && rays * k / G < (double)c->opt.merge_rays) k *= 2u;
        return k;
    };
    for (uint32_t b = 0; b < mb; b++) {
        uint32_t* q = R.queue[b & 1]; uint32_t* qn = R.queue[(b + 1) & 1];
        DevPaths Pb = P;                                  // compact state: bounce b reads set (b & 1) and writes the survivors into the other one
        if (compact) {
            F4* set[2][3] = {{(F4*)c->pt.d_ray_o.p, (F4*)c->pt.d_ray_d.p, (F4*)c->pt.d_thr.p}, {(F4*)c->pt.d_alt_o.p, (F4*)c->pt.d_alt_d.p, (F4*)c->pt.d_alt_thr.p}};
            Pb.ray_o = set[b & 1][0]; Pb.ray_d = set[b & 1][1]; Pb.thr = set[b & 1][2];
            Pb.out_o = set[(b + 1) & 1][0]; Pb.out_d = set[(b + 1) & 1][1]; Pb.out_thr = set[(b + 1) & 1][2];
            if (osort) {           // shade(b) notes the survivors' octants for bounce b + 1; trace(b), b >= 1, sorts by what shade(b - 1) noted (camera rays of one block share their octant anyway)
                Pb.oct_out = c->opt.octant_sort == 2 ? nullptr : (uint8_t*)c->pt.d_oct[(b + 1) & 1].p;
                if (b >= (c->opt.octant_sort == 3 ? 2u : 1u)) { Pb.oct_in = (const uint8_t*)c->pt.d_oct[b & 1].p; Pb.perm = (uint32_t*)c->pt.d_perm.p; }     // (origin cells: bounce 1 starts at the camera rays' hits, already in image order)
            }
        }
        DevScene scb = c->dsc;
        if (c->scene.wide_nodes && b >= 1u) { scb.nodes_f = (const F4*)c->scene.d_nodes_wide.p; scb.node_v4 = 8u; }
        if (c->scene.lds_nodes_closest) scb.lds_nodes = c->scene.lds_nodes_closest;          // closest-hit launches stage more of the tree's top than the shadow launches (finalise_scene)
        { Timed t(c, RTX_K_TRACE); launch_trace_closest(st, fb, scb, Pb, b, q, R.Q(b), Hd(b, 0), merge_for(b < c->pt.pred_q.size() ? c->pt.pred_q[b] : 0, b < c->pt.pred_q.size())); }
        if (ovl && ev_shadow_done) HIPCHK(c, hipStreamWaitEvent(st, ev_shadow_done, 0));      // shade(b) overwrites the shadow entries and touches rad: after shadow(b - 1)
        { Timed t(c, RTX_K_SHADE); launch_shade(st, c->dsc, fb, Pb, b, q, R.Q(b), qn, R.Q(b + 1), R.S(b, 0)); }
        hipStream_t ss = st;
        if (ovl && nee) {
            hipEvent_t e = c->ev.take(); ev_shadow_done = c->ev.take();
            if (!e || !ev_shadow_done) { c->err = "render: out of events"; return RTX_ERR_HIP; }
            HIPCHK(c, hipEventRecord(e, st)); HIPCHK(c, hipStreamWaitEvent(c->pt.aux, e, 0));
            ss = c->pt.aux;
        }
        for (uint32_t j = 0; j < nee; j++) { const size_t ps = (size_t)b * nee1 + j; Timed t(c, RTX_K_SHADOW, ss); launch_trace_shadow(ss, fb, c->dsc, Pb, j, R.S(b, j), Hd(b, 1 + j), merge_for(ps < c->pt.pred_s.size() ? c->pt.pred_s[ps] : 0, ps < c->pt.pred_s.size() && c->pt.pred_nee1 == nee1)); }
        if (ovl && nee) HIPCHK(c, hipEventRecord(ev_shadow_done, c->pt.aux));
    }
    if (ovl && ev_shadow_done) HIPCHK(c, hipStreamWaitEvent(st, ev_shadow_done, 0));
    return RTX_OK;
}

}  // namespace

extern "C" {

int rtx_render(rtx_ctx* c, const rtx_params* p) {
    // ---- 1. validate ----
    DevFrame f;
    int r = render_checks(c, p, false, f);
    if (r) return r;
    if ((r = ensure_accum(c, p->width, p->height, false))) return r;
    stats_begin(c);
    if (p->spp == 0) return RTX_OK;
    c->ad.pure = false;                        // u1 now holds samples that `half` does not know: rtx_render_adaptive refuses until the next clear
    if ((r = render_frame(c, p, f, p->spp, nullptr))) return r;
    // RTX_OPT_ASYNC on a caller-bound stream: the frame is enqueued, the caller goes on enqueueing its epilogue (rtx_pack_tiles -> collective -> rtx_unpack_tiles) behind it
    // with no host join in between; statistics and the launch-size predictions of the next frame are collected at the next call that needs them (BIND)
    if (c->opt.async && !c->own_stream) return RTX_OK;
    return finish_render(c);
}

}  // extern "C"

// steps 2 - 5 of a frame: `spp` samples for every slot of the frame, enqueued; finish_render collects.  lp: a pass of rtx_render_adaptive — the slots are those of the active
// list (a virtual frame of 256 n_active slots that is planned, sized and dealt like a small shard), sample ids start at lp->sample_first, the accumulation is the adaptive form
int render_frame(rtx_ctx* c, const rtx_params* p, const DevFrame& f_real, uint32_t spp, const ListPass* lp) {
    int r = RTX_OK;
    DevFrame f = f_real;
    if (lp) { f.list = lp->list; f.npl = lp->n_active * 256u; f.chunks_per_sample = lp->n_active; }
    const uint32_t sample_first = lp ? lp->sample_first : p->sample_base;

    // ---- 2. plan the batches ----
    // NEE slots: nee_samples towards the triangle lights, then one towards an environment that has weight (k_shade<.., ENV>: shadow queue, counters and launch follow the others')
    const uint32_t nee = (c->dsc.nlights ? p->nee_samples : 0) + (c->dsc.env_tex ? 1u : 0u);
    const bool tiny_fused = c->dsc.nsmall && c->opt.fused;
    // (the other wave schedules are experiment knobs of the separate kernels; with a texture map active the separate kernels run whatever the option says: k_bounce_bvh samples no image)
    const bool fused_bvh = !c->dsc.nsmall && c->opt.fused_bvh && c->opt.trace_sched >= 5u && !c->dsc.tri_uv && !c->dsc.tri_cut && !c->dsc.env_n;
    const BatchPlan B = plan_batches(c, spp, f, fused_bvh);
    const uint32_t bspp = B.bspp, G = B.G;
    const uint64_t cap64 = (uint64_t)f.npl * bspp;
    if (cap64 > 0x7FFFFFFFull) { c->err = "render: batch too large"; return RTX_ERR_INVALID; }
    const uint32_t cap = (uint32_t)cap64;

    // ---- 3. size the buffers ----
    HIPCHK(c, c->pt.d_rad.ensure((size_t)cap * 16));
    const uint32_t qcap = B.qchunks * 256u;
    f.nblocks = G; f.qcap = qcap; f.taper_levels = B.taper_levels;
    const size_t qtot = (size_t)G * qcap;
    // path state: by path id (cap entries), or — the default configuration — by queue position (qtot >= cap entries) in two sets.  The separate kernels get their second set
    // in buffers of its own (d_alt_*, handed over per bounce: enqueue_bounces); the fused tiny-scene kernels, which run all bounces >= 1 in one launch, find it `nstate` entries
    // behind the first in the SAME three allocations: one scalar toggles per bounce instead of six pointers (k_bounce_small spills SGPRs as it is)
    const size_t nstate = B.compact ? qtot : (size_t)cap;
    const bool tiny_compact = tiny_fused && B.compact;
    const size_t nsets = tiny_compact ? 2 : 1;
    if (nstate * nsets > 0xFFFFFFFFull) { c->err = "render: batch too large"; return RTX_ERR_INVALID; }
    HIPCHK(c, c->pt.d_ray_o.ensure(nstate * nsets * 16)); HIPCHK(c, c->pt.d_ray_d.ensure(nstate * nsets * 16)); HIPCHK(c, c->pt.d_thr.ensure(nstate * nsets * 16));
    HIPCHK(c, c->pt.d_hit.ensure((tiny_fused ? (size_t)cap : nstate) * 16));          // (tiny scenes: the primary hits, by path id)
    if (B.compact && !tiny_fused) { HIPCHK(c, c->pt.d_alt_o.ensure(nstate * 16)); HIPCHK(c, c->pt.d_alt_d.ensure(nstate * 16)); HIPCHK(c, c->pt.d_alt_thr.ensure(nstate * 16)); }
    HIPCHK(c, c->pt.d_queue[0].ensure(qtot * 4)); HIPCHK(c, c->pt.d_queue[1].ensure(qtot * 4));
    HIPCHK(c, c->pt.d_order.ensure((size_t)G * 4));
    if (fused_bvh) HIPCHK(c, c->pt.d_hitq.ensure(qtot * 4));
    FrameRun R{};
    R.G = G; R.mb = p->max_bounces; R.nee = nee; R.nee1 = std::max<uint32_t>(nee, 1); R.compact = B.compact;
    R.stealing = !c->dsc.nsmall && !fused_bvh && c->opt.work_stealing && !c->dsc.tri_cut && p->max_bounces > 0;      // (no stealing instantiation has a CUT form)
    R.hstride = (size_t)G + (G + 31) / 32;                                   // per trace launch: G fetch cursors + the exhausted bitmap
    R.nheads = R.stealing ? (size_t)p->max_bounces * (1 + std::max<uint32_t>(nee, 1)) * R.hstride : 0;
    if (R.stealing) HIPCHK(c, c->pt.d_heads.ensure(R.nheads * 4));
    HIPCHK(c, c->pt.d_pmask.ensure(((size_t)f_real.npl / 64 + 1) * 8));        // (per real slot, like the shared-primary records: computed once per call)
    // RTX_OPT_SHARED_PRIMARY: without jitter the camera ray of a pixel is the same for every sample, so the fused tiny-scene path traces and reconstructs it once per call
    // A THIN LENS (rtx_set_lens, radius > 0) ends both: every sample starts at its own point of the aperture, so no two samples of a pixel share a ray — no shared primary hit,
    // whatever the option says — and the pyramid of a block's corner rays from the camera origin does not bound them — no packet culling: every mask word is all ones
    const bool lens = f_real.lens_radius > 0.0f;
    const bool shared_primary = tiny_fused && c->opt.shared_primary && !(p->flags & RTX_FLAG_JITTER) && !lens;
    if (shared_primary) { HIPCHK(c, c->pt.d_prim_rec.ensure(((size_t)f_real.npl * 3 + 1) * 16)); HIPCHK(c, c->pt.d_prim_hits.ensure(((size_t)f_real.npl / 64 * 2 + 1) * 8)); }
    R.prim_rec = shared_primary ? (const F4*)c->pt.d_prim_rec.p : nullptr; R.rec_npl = f_real.npl;
    const size_t shn = qtot * R.nee1;
    HIPCHK(c, c->pt.d_sh_o.ensure(shn * 16)); HIPCHK(c, c->pt.d_sh_d.ensure(shn * 16)); HIPCHK(c, c->pt.d_sh_c.ensure(shn * 16));
    DevPaths& P = R.P;
    P.ray_o = (F4*)c->pt.d_ray_o.p; P.ray_d = (F4*)c->pt.d_ray_d.p; P.thr = (F4*)c->pt.d_thr.p; P.rad = (F4*)c->pt.d_rad.p; P.hit = (F4*)c->pt.d_hit.p;
    P.hitmask = nullptr;
    P.out_o = P.out_d = P.out_thr = nullptr;
    if (tiny_compact) { P.out_o = P.ray_o + nstate; P.out_d = P.ray_d + nstate; P.out_thr = P.thr + nstate; }      // the same distance in all three streams (state_set_stride)
    P.oct_out = nullptr; P.oct_in = nullptr; P.perm = nullptr; P.key_mode = (uint32_t)c->opt.octant_sort;
    R.osort = c->opt.octant_sort && B.compact && !tiny_fused && !R.stealing;
    if (R.osort) { HIPCHK(c, c->pt.d_oct[0].ensure(qtot)); HIPCHK(c, c->pt.d_oct[1].ensure(qtot)); HIPCHK(c, c->pt.d_perm.ensure(qtot * 4)); }
    if (R.osort && c->opt.octant_sort == 2) { HIPCHK(c, hipMemsetAsync(c->pt.d_oct[0].p, 0, qtot, c->stream)); HIPCHK(c, hipMemsetAsync(c->pt.d_oct[1].p, 0, qtot, c->stream)); }
    if (tiny_fused && !shared_primary) { HIPCHK(c, c->pt.d_hitmask.ensure(((size_t)cap / 64 + 1) * 8)); P.hitmask = (unsigned long long*)c->pt.d_hitmask.p; }
    P.sh_o = (F4*)c->pt.d_sh_o.p; P.sh_d = (F4*)c->pt.d_sh_d.p; P.sh_c = (F4*)c->pt.d_sh_c.p;
    R.queue[0] = (uint32_t*)c->pt.d_queue[0].p; R.queue[1] = (uint32_t*)c->pt.d_queue[1].p;
    const uint32_t mb = R.mb, nee1 = R.nee1;
    const size_t ncnt = ((size_t)(mb + 1) + (size_t)mb * nee1 + 1) * G;    // (FrameRun: Q rows, S rows, + one row: paths generated)
    const uint32_t nbatches = (spp + bspp - 1) / bspp;
    HIPCHK(c, c->pt.d_counters.ensure(ncnt * 4));
    HIPCHK(c, c->pt.h_counters.ensure(ncnt * nbatches * 4));
    R.cnt = (uint32_t*)c->pt.d_counters.p;
    R.cam = (const CameraGPU*)c->d_cam.p;
    c->ev.used = 0; c->timed.clear();
    const hipStream_t st = R.st = c->stream;

    // ---- 4. enqueue the batches ----
    // every early return below (HIPCHK) must not leave shadow-ray launches of the internal `aux` stream running behind the caller's back: they read the
    // shadow entries and update `rad`, which the next call re-uses
    struct AuxJoin { rtx_ctx* c; bool armed = true; ~AuxJoin() { if (armed && c->pt.aux) (void)hipStreamSynchronize(c->pt.aux); } } aux_join{c};
    HIPCHK(c, hipEventRecord(c->ev.begin, st));
    HIPCHK(c, hipMemsetAsync(R.cnt, 0, ncnt * 4, st));
    // per 8x8 block resp. per pixel, shared by all samples and batches of this call; recomputed every call (camera, scene, size and shard may all have changed)
    const bool tables_in_place = lp && !lp->first;             // a later pass of the same rtx_render_adaptive call
    if (shared_primary && !tables_in_place) { Timed t(c, RTX_K_RAYGEN); launch_primary_surface(st, c->dsc, f_real, R.cam, (unsigned long long*)c->pt.d_pmask.p, (unsigned long long*)c->pt.d_prim_hits.p, (F4*)c->pt.d_prim_rec.p); }
    else if (tiny_fused && !tables_in_place) {
        if (lens) HIPCHK(c, hipMemsetAsync(c->pt.d_pmask.p, 0xFF, ((size_t)f_real.npl / 64 + 1) * 8, st));      // keep every record (traverse_small masks the bits at and above nsmall itself, as for its default ~0)
        else launch_packet_masks(st, c->dsc, f_real, R.cam, (unsigned long long*)c->pt.d_pmask.p);
    }
    for (uint32_t bi = 0; bi < nbatches; bi++) {
        DevFrame fb = f;
        fb.sample_first = sample_first + bi * bspp;
        fb.batch_spp = std::min(bspp, spp - bi * bspp);
        fb.interleave = 0;                                     // (k_raygen only: the tiny-scene raygen keeps its packet order)
        if (c->opt.sample_interleave) while (fb.interleave < 4u && !((fb.batch_spp >> fb.interleave) & 1u)) fb.interleave++;       // S = the largest power of two <= 16 dividing the batch's sample count
        r = tiny_fused ? enqueue_tiny_fused(c, R, fb) : fused_bvh ? enqueue_fused_bvh(c, R, fb) : enqueue_bounces(c, R, fb);
        if (r) return r;
        // ---- 5. accumulate, copy the counters ----
        { Timed t(c, RTX_K_ACCUM); const unsigned long long* ph = shared_primary ? (const unsigned long long*)c->pt.d_prim_hits.p : nullptr;      // (one hit mask per block for all samples; P.hitmask is null then)
          if (lp) launch_accumulate_list(st, B.max_blocks, fb, P, c->accum_ptr(), lp->state, ph); else launch_accumulate(st, B.max_blocks, fb, P, c->accum_ptr(), ph); }
        HIPCHK(c, hipMemcpyAsync(c->pt.h_counters.as<uint32_t>() + (size_t)bi * ncnt, R.cnt, ncnt * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(c, hipEventRecord(c->ev.end, st));
    HIPCHK(c, hipGetLastError());
    aux_join.armed = false;                    // the main stream waited for the last shadow launch (ev_shadow_done) before the accumulation: stream order covers the aux stream
    c->pt.pending.active = true; c->pt.pending.ncnt = ncnt; c->pt.pending.nbatches = nbatches; c->pt.pending.G = G; c->pt.pending.mb = mb; c->pt.pending.nee = nee; c->pt.pending.nee1 = nee1;
    c->pt.pending.fused = tiny_fused; c->pt.pending.fused_bvh = fused_bvh;
    return RTX_OK;
}

// the kernel times of the launches bracketed since the last collection (RTX_OPT_KERNEL_TIMING); the stream must have passed them
void collect_timed(rtx_ctx* c) {
    for (const TimedLaunch& t : c->timed) { float m = 0.0f; if (hipEventElapsedTime(&m, t.a, t.b) == hipSuccess) c->stats.kernel_ms[t.cls] += m; }
    c->timed.clear();
}

int finish_render(rtx_ctx* c) {
    if (!c->pt.pending.active) return RTX_OK;
    c->pt.pending.active = false;
    const size_t ncnt = c->pt.pending.ncnt; const uint32_t nbatches = c->pt.pending.nbatches, G = c->pt.pending.G, mb = c->pt.pending.mb, nee = c->pt.pending.nee, nee1 = c->pt.pending.nee1;
    const bool fused = c->pt.pending.fused, fused_bvh = c->pt.pending.fused_bvh;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev.begin, c->ev.end) == hipSuccess) c->stats.render_ms += ms;      // (summed over the passes of rtx_render_adaptive; rtx_render starts from zero)
    collect_timed(c);
    if (!fused && !fused_bvh) { c->pt.pred_paths = 0; c->pt.pred_q.assign(mb, 0); c->pt.pred_s.assign((size_t)mb * nee1, 0); c->pt.pred_nee1 = nee1; }
    for (uint32_t bi = 0; bi < nbatches; bi++) {
        const uint32_t* h = c->pt.h_counters.as<uint32_t>() + (size_t)bi * ncnt;
        auto sumG = [&](size_t row) { uint64_t s = 0; for (uint32_t g = 0; g < G; g++) s += h[row * G + g]; return s; };
        if (!fused && !fused_bvh) {                 // what the next call's launches are sized by (merge_for)
            c->pt.pred_paths += sumG(0);
            for (uint32_t b = 0; b < mb; b++) { c->pt.pred_q[b] += sumG(b); for (uint32_t j = 0; j < nee1; j++) c->pt.pred_s[(size_t)b * nee1 + j] += sumG((size_t)(mb + 1) + (size_t)b * nee1 + j); }
        }
        const uint64_t prim = fused ? sumG((size_t)(mb + 1) + (size_t)mb * nee1) : sumG(0);
        c->stats.rays_primary += prim; c->stats.paths += prim;
        c->stats.primary_hits += fused ? sumG(0) : 0;
        for (uint32_t b = 1; b < mb; b++) c->stats.rays_extension += sumG(b);
        for (uint32_t b = 0; b < mb; b++) for (uint32_t j = 0; j < nee; j++) c->stats.rays_shadow += sumG((size_t)(mb + 1) + (size_t)b * nee1 + j);
    }
    c->stats.kernel_items[RTX_K_RAYGEN] = c->stats.paths;
    c->stats.kernel_items[RTX_K_BOUNCE] = fused ? c->stats.primary_hits + c->stats.rays_extension : fused_bvh ? c->stats.rays_primary + c->stats.rays_extension : 0;   // tiny scenes: bounce 0 shades the primary hits only
    c->stats.kernel_items[RTX_K_TRACE] = (fused || fused_bvh) ? 0 : c->stats.rays_primary + c->stats.rays_extension;
    c->stats.kernel_items[RTX_K_SHADE] = (fused || fused_bvh) ? 0 : c->stats.rays_primary + c->stats.rays_extension;
    c->stats.kernel_items[RTX_K_SHADOW] = (fused || fused_bvh) ? 0 : c->stats.rays_shadow;
    c->stats.kernel_items[RTX_K_ACCUM] = c->stats.paths;
    return RTX_OK;
}

// rtx_restir_api.hip — the ReSTIR frames (rtx_render_v6_pass1, rtx_render_restir): the wavefront stages of the three passes over work lists, run as independent lanes; on
// shards, the exchange of the history (whole own tiles, or border strips only).  Part of the C-ABI of include/rtx.h (rtx_ctx.hpp).
#include "rtx_ctx.hpp"

extern "C" {

size_t rtx_pass1_slots(uint32_t w, uint32_t h) { return (size_t)((w + 3) / 4) * ((h + 3) / 4) * 16; }
static int p1_alloc(rtx_ctx* c, size_t slots);

// ---- the ReSTIR passes as wavefront stages (csrc/rtx_restir_wave.hpp) ----------------------------------------------------------------------------------
// One pass at a time owns the work area.  `nitems` work items (pixels of the shard's own tiles, or — passes 1 and 2 on shards — of the dilated tiles) are cut
// into 256-item chunks and dealt round-robin to G workgroups, each with a private sub-queue: stage kernels and the persistent traversal kernels of a pass all run
// with G workgroups, workgroup b owning sub-queue b.  G: `restir_chunks` chunks per workgroup (more = fuller persistent waves, fewer = shorter launch tails).
struct RsPlan { RsQ q; uint32_t* cnt; uint32_t G; DevFrame fq; DevPaths P[2]; };
static int rs_plan(rtx_ctx* c, const DevFrame& f, uint32_t nitems, const uint32_t* pixels, uint32_t rows, RsPlan& R, uint32_t lane) {
    rtx_ctx::Restir::RsArea& A = c->rs.rs_area[lane];
    const uint32_t nchunks = std::max<uint32_t>(1u, (nitems + 255u) / 256u);
    // `restir_chunks` chunks per workgroup at full frame size, but never fewer than ~8 workgroups per CU while there are that many chunks: a 1/8 shard (1 180 chunks with its
    // halo) ran 3.63 ms per frame with 295 workgroups of 4 chunks and 2.22 ms with 1 180 of one (tools/shard_time.py sponza restir 8 blocks=1 tile=32)
    const uint32_t want = std::max<uint32_t>((nchunks + c->opt.restir_chunks - 1) / c->opt.restir_chunks, (uint32_t)c->num_cus * 8u);
    const uint32_t G = (std::max<uint32_t>(1u, std::min<uint32_t>(std::min<uint32_t>(want, nchunks), (uint32_t)c->num_cus * 64u)) + 7u) & ~7u;   // a multiple of 8: rs_wg() maps workgroups to XCD-contiguous ranges
    const uint32_t qcap = ((nchunks + G - 1) / G) * 256u, rcap = qcap * 9u;              // a pixel casts at most 9 visibility rays in one stage (pass 3, select)
    const size_t qtot = (size_t)G * qcap, rtot = (size_t)G * rcap;
    // 32-bit indices everywhere: queue positions (rtot), the per-item candidate / cold records, and the ray payload `item * kRsOcc + k` that addresses the occlusion bytes
    // (rs_push_ray: a wrapped payload would write the verdict of ANOTHER pixel's ray, silently)
    if (rtot > 0xFFFFFFFFull || (uint64_t)nitems * kRsOcc > 0xFFFFFFFFull || (uint64_t)nitems * kRsCand > 0xFFFFFFFFull || (uint64_t)nitems * 5u > 0xFFFFFFFFull) {
        c->err = "render_restir: image too large (32-bit ray payloads and record indices)"; return RTX_ERR_INVALID;
    }
    HIPCHK(c, A.state.ensure(qtot * 16 * 2 * kRsStreams)); HIPCHK(c, A.hit.ensure(qtot * 16));
    HIPCHK(c, A.cls.ensure((size_t)nitems * 4)); HIPCHK(c, A.fin.ensure((size_t)nitems * 16)); HIPCHK(c, A.cold.ensure((size_t)nitems * 16 * 5));
    HIPCHK(c, A.occ.ensure((size_t)nitems * kRsOcc)); HIPCHK(c, A.cand.ensure((size_t)nitems * 4 * kRsCand));
    HIPCHK(c, A.sho.ensure(rtot * 16)); HIPCHK(c, A.shd.ensure(rtot * 16)); HIPCHK(c, A.pay.ensure(rtot * 4));
    HIPCHK(c, A.cnt.ensure((size_t)rows * G * 4));
    RsQ& q = R.q;
    q.nitems = nitems; q.pixels = pixels; q.G = G; q.qcap = qcap; q.rcap = rcap;
    for (uint32_t set = 0; set < 2; set++) for (uint32_t k = 0; k < kRsStreams; k++) q.st[set][k] = (F4*)A.state.p + ((size_t)set * kRsStreams + k) * qtot;
    q.hit = (F4*)A.hit.p; q.cls = (uint32_t*)A.cls.p; q.fin = (F4*)A.fin.p; q.cold = (F4*)A.cold.p;
    q.occ = (uint8_t*)A.occ.p; q.cand = (uint32_t*)A.cand.p;
    q.sh_o = (F4*)A.sho.p; q.sh_d = (F4*)A.shd.p; q.sh_pay = (uint32_t*)A.pay.p;
    q.rays = (unsigned long long*)c->rs.d_p1cnt.p;
    R.cnt = (uint32_t*)A.cnt.p; R.G = G;
    R.fq = f; R.fq.nblocks = G; R.fq.qcap = qcap;
    for (uint32_t set = 0; set < 2; set++) {          // what k_trace_closest sees of a set: rays and hit records by queue position ("compact state": out_o != nullptr is the flag)
        DevPaths P{}; P.ray_o = q.st[set][0]; P.ray_d = q.st[set][1]; P.hit = q.hit; P.out_o = q.st[set ^ 1u][0];
        R.P[set] = P;
    }
    return RTX_OK;
}
// pass 1 of one sample (RayGen_v6_pass1.hlsl:48-190): raygen | trace | ris | trace | ris_finish | trace | first | (trace | loop) x bounces | emit_final | trace | finish.
// bufs != nullptr (a ReSTIR frame): pass 2 (RayGen_v6_pass2.hlsl:46-204) rides on the last two stages.  Everything is enqueued on `st` with the work area of `lane`.
static int rs_pass1(rtx_ctx* c, const DevFrame& f, uint32_t sample_id, F4* accum, const uint32_t* pixels, uint32_t npixels, uint32_t* const* bufs, uint32_t lane, hipStream_t st) {
    const uint32_t mb = f.max_bounces, rows = 4u + mb + 1u;
    RsPlan R; int r = rs_plan(c, f, pixels ? npixels : f.npl, pixels, rows, R, lane); if (r) return r;
    DevScene sc = c->plain_scene(); sc.tri_cut = nullptr; const RsQ& q = R.q;      // (the ReSTIR frame ignores alpha cut-outs, as it ignores map_Kd: its closest-hit launches are the plain instantiations)
    const CameraGPU* cam = (const CameraGPU*)c->d_cam.p;
    auto row = [&](uint32_t k) { return R.cnt + (size_t)k * R.G; };
    uint32_t* res_di = (uint32_t*)c->rs.d_res_di.p; uint32_t* res_gi = (uint32_t*)c->rs.d_res_gi.p; uint32_t* sdata = (uint32_t*)c->rs.d_sdata.p;
    uint32_t* shrow = row(4 + mb);                          // lengths of the ray sub-queues: DI visibility (stage 2) + reconnection + temporal rays (stage 5)
    { Timed t(c, RTX_K_RAYGEN, st); launch_rs_raygen(st, R.fq, q, cam, sample_id, row(0)); }
    { Timed t(c, RTX_K_TRACE, st); launch_trace_closest(st, R.fq, sc, R.P[0], 0, nullptr, row(0), nullptr); }                    // camera rays (tmin 1e-4)
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_ris(st, sc, R.fq, q, row(0), row(1), accum, res_di, res_gi, sdata); }
    { Timed t(c, RTX_K_TRACE, st); launch_trace_closest(st, R.fq, sc, R.P[1], 1, nullptr, row(1), nullptr); }                    // the BSDF candidates of SampleRIS
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_ris_finish(st, sc, R.fq, q, row(1), row(2), shrow, res_di, sdata); }
    { Timed t(c, RTX_K_TRACE, st); launch_trace_closest(st, R.fq, sc, R.P[0], 1, nullptr, row(2), nullptr); }                    // first path vertex
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_first(st, sc, R.fq, q, row(2), row(3)); }
    for (uint32_t i = 0; i < mb; i++) {
        const uint32_t set = (i + 1u) & 1u;                 // k_rs_p1_first wrote set 1
        { Timed t(c, RTX_K_TRACE, st); launch_trace_closest(st, R.fq, sc, R.P[set], 1, nullptr, row(3 + i), nullptr); }
        { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_loop(st, sc, R.fq, q, set, i, row(3 + i), row(4 + i)); }
    }
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_emit_final(st, sc, R.fq, q, cam, bufs, shrow); }
    { Timed t(c, RTX_K_SHADOW, st); launch_trace_occ(st, sc, q, shrow); }                                                        // DI visibility, the selected reconnection, the temporal pass's two rays
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p1_finish(st, sc, R.fq, q, accum, res_di, res_gi, sdata, cam, bufs); }
    if (bufs && c->opt.restir_keys) { Timed t(c, RTX_K_SHADE, st); launch_rs_p3_keys(st, R.fq, q, bufs, (F4*)c->rs.d_rs_key_a.p, (F4*)c->rs.d_rs_key_b.p); }      // what the spatial pass's neighbour tests read
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}
static int rs_pass3(rtx_ctx* c, const DevFrame& f, uint32_t* const bufs[6], F4* accum, const uint32_t* pixels, uint32_t npixels, uint32_t lane, hipStream_t st) {
    RsPlan R; int r = rs_plan(c, f, pixels ? npixels : f.npl, pixels, 2, R, lane); if (r) return r;
    const CameraGPU* cam = (const CameraGPU*)c->d_cam.p;
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p3_select(st, c->plain_scene(), R.fq, R.q, cam, bufs, R.cnt, c->opt.restir_keys ? (F4*)c->rs.d_rs_key_a.p : nullptr, c->opt.restir_keys ? (F4*)c->rs.d_rs_key_b.p : nullptr); }
    { Timed t(c, RTX_K_SHADOW, st); launch_trace_occ(st, c->plain_scene(), R.q, R.cnt); }
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p3_merge(st, c->plain_scene(), R.fq, R.q, bufs, R.cnt + R.G); }
    { Timed t(c, RTX_K_SHADOW, st); launch_trace_occ(st, c->plain_scene(), R.q, R.cnt + R.G); }
    { Timed t(c, RTX_K_SHADE, st); launch_rs_p3_shade(st, c->plain_scene(), R.fq, R.q, bufs, accum); }
    HIPCHK(c, hipGetLastError());
    return RTX_OK;
}
// One pass over a work list as `lanes` independent parts: part 0 on the context's stream, part 1 on the internal stream, joined at the end.  A ReSTIR frame is ~20 short,
// dependent launches; run as ONE chain every launch drains before the next ramps up (k_trace_* at 4.8-5.0 of 8 waves per SIMD, VALU pipes 0.82 busy: profiles/r03_pmc_restir.md).
// Pixels are independent inside passes 1 + 2 and inside pass 3, so two chains over the two halves of the list fill each other's tails.  Not while kernels are timed.
extern "C++" {
template <class F>
static int rs_lanes(rtx_ctx* c, const uint32_t* pixels, uint32_t npixels, F&& pass) {
    const uint32_t L = (pixels && !c->opt.timing && npixels >= c->opt.restir_lane_min) ? c->opt.restir_lanes : 1u;
    if (L <= 1u) return pass(pixels, npixels, 0u, c->stream);
    hipEvent_t e0 = c->ev.take();
    if (!e0) { c->err = "render_restir: out of events"; return RTX_ERR_HIP; }
    HIPCHK(c, hipEventRecord(e0, c->stream));
    const uint32_t part = (((npixels + L - 1u) / L) + 255u) & ~255u;          // whole chunks
    for (uint32_t l = 0; l < L; l++) {
        const uint32_t lo = std::min(npixels, l * part), hi = std::min(npixels, (l + 1u) * part);
        if (lo == hi) continue;
        hipStream_t st = c->stream;
        if (l) {
            if (!c->rs.lane_stream[l - 1]) c->rs.lane_stream[l - 1] = c->streams.set.s[1 + l];
            st = c->rs.lane_stream[l - 1];
            HIPCHK(c, hipStreamWaitEvent(st, e0, 0));
        }
        int r = pass(pixels + lo, hi - lo, l, st); if (r) return r;
        if (l) { hipEvent_t e = c->ev.take(); if (!e) { c->err = "render_restir: out of events"; return RTX_ERR_HIP; } HIPCHK(c, hipEventRecord(e, st)); HIPCHK(c, hipStreamWaitEvent(c->stream, e, 0)); }
    }
    return RTX_OK;
}
}  // extern "C++"
static void stats_end_restir(rtx_ctx* c, const unsigned long long cnt[3]) {
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, c->ev.begin, c->ev.end) == hipSuccess) c->stats.render_ms = ms;
    collect_timed(c);
    c->stats.rays_primary = cnt[0]; c->stats.rays_extension = cnt[1]; c->stats.rays_shadow = cnt[2]; c->stats.paths = cnt[0]; c->stats.primary_hits = 0;
    c->stats.kernel_items[RTX_K_RAYGEN] = cnt[0]; c->stats.kernel_items[RTX_K_TRACE] = cnt[0] + cnt[1]; c->stats.kernel_items[RTX_K_SHADOW] = cnt[2];
}

int rtx_render_v6_pass1(rtx_ctx* c, const rtx_params* p) {
    DevFrame f;
    int r = render_checks(c, p, true, f);
    if (r) return r;
    if ((r = ensure_accum(c, p->width, p->height, false))) return r;
    c->ad.pure = false;                        // (rtx_render_adaptive: u1 gets samples its second sum does not hold)
    const size_t slots = rtx_pass1_slots(p->width, p->height);
    if ((r = p1_alloc(c, slots))) return r;
    stats_begin(c);
    HIPCHK(c, hipMemsetAsync(c->rs.d_p1cnt.p, 0, 24, c->stream));
    HIPCHK(c, hipEventRecord(c->ev.begin, c->stream));
    for (uint32_t s = 0; s < p->spp; s++) {
        if (c->opt.restir_wave) { if ((r = rs_pass1(c, f, p->sample_base + s, c->accum_ptr(), nullptr, 0, nullptr, 0u, c->stream))) return r; }
        else { Timed t(c, RTX_K_BOUNCE);
               launch_v6_pass1(c->stream, (uint32_t)c->num_cus * 8u, c->plain_scene(), f, (const CameraGPU*)c->d_cam.p, p->sample_base + s, c->accum_ptr(),
                               (uint32_t*)c->rs.d_res_di.p, (uint32_t*)c->rs.d_res_gi.p, (uint32_t*)c->rs.d_sdata.p, (unsigned long long*)c->rs.d_p1cnt.p); }
    }
    HIPCHK(c, hipEventRecord(c->ev.end, c->stream));
    HIPCHK(c, hipGetLastError());
    unsigned long long cnt[3] = {0, 0, 0};
    TO_HOST(c, cnt, c->rs.d_p1cnt.p, 24);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    stats_end_restir(c, cnt);
    return RTX_OK;
}

static int p1_alloc(rtx_ctx* c, size_t slots) {
    HIPCHK(c, c->rs.d_res_di.ensure(slots * 40)); HIPCHK(c, c->rs.d_res_gi.ensure(slots * 40)); HIPCHK(c, c->rs.d_sdata.ensure(slots * 60));
    HIPCHK(c, c->rs.d_p1cnt.ensure(32));          // rays by type (3 x u64) + stale history reads
    if (c->rs.p1_slots != slots) {
        HIPCHK(c, hipMemsetAsync(c->rs.d_res_di.p, 0, slots * 40, c->stream)); HIPCHK(c, hipMemsetAsync(c->rs.d_res_gi.p, 0, slots * 40, c->stream));
        HIPCHK(c, hipMemsetAsync(c->rs.d_sdata.p, 0, slots * 60, c->stream));
        c->rs.p1_slots = slots;
    }
    return RTX_OK;
}

int rtx_restir_reset(rtx_ctx* c) {
    BIND(c);
    c->rs.last_slots = 0;           // the next frame starts from zeroed g_*_last buffers
    c->rs.hist_all = true;          // ... which is what every rank holds then: valid everywhere
    return RTX_OK;
}

int rtx_render_restir(rtx_ctx* c, const rtx_params* p) {
    DevFrame f;
    int r = render_checks(c, p, true, f);
    if (r) return r;
    // ReSTIR ON SHARDS (shard_count > 1).  The spatial pass of a pixel reads this frame's pass-1 / pass-2 records of neighbours within 20 px
    // (RayGen_v6_pass3.hlsl:46-372) and the temporal pass reads last frame's history at an arbitrary reprojected pixel (RayGen_v6_pass2.hlsl:46-204).  So a shard
    //   * runs passes 1 and 2 on its tiles DILATED by 20 px (the halo is recomputed: seeds depend on the pixel only, results are what the owner computes),
    //   * runs pass 3 (and the accumulation) on its own tiles,
    //   * and after the frame the shards exchange the history of their own tiles: rtx_restir_pack_state -> one all-gather -> rtx_restir_unpack_state,
    // which the caller does between frames — hence one frame per call.  Images and histories are bit-identical to the unsharded run.
    // With RTX_FLAG_BLOCK_TILES the tiles of a shard form ONE rectangle, so the dilation adds a 20-px rim (8 shards at 1080p: 1.16 x the own pixels) instead of a rim
    // around every 64-px tile (2.6 x with the round-robin deal).
    const bool sharded = p->shard_count > 1;
    if (sharded && p->spp != 1) { c->err = "render_restir: on shards the history has to be exchanged after every frame (rtx_restir_pack_state / unpack_state): spp must be 1"; return RTX_ERR_INVALID; }
    if ((r = ensure_accum(c, p->width, p->height, false))) return r;
    c->ad.pure = false;                        // (rtx_render_adaptive: u1 gets samples its second sum does not hold)
    const uint32_t* halo = nullptr; const uint32_t* own = nullptr; uint32_t nhalo = 0, nown = 0;
    // (tiny scenes keep the slot order when unsharded: the Cornell frame measured 3.19 ms that way and 3.69 ms through the Morton list; the BVH scenes gain ~1 %)
    if (sharded || (c->opt.restir_wave && !c->dsc.nsmall)) {
        const uint32_t key[6] = {p->width, p->height, f.tile_size, p->shard_rank, f.shard_count, p->flags & RTX_FLAG_BLOCK_TILES};
        if (memcmp(key, c->rs.halo_key, sizeof(key)) != 0 || !c->rs.d_own.p) {
            const uint32_t W = p->width, H = p->height, ts = f.tile_size, R = 20u;           // spatial radius: RayGen_v6_pass3.hlsl (random pixel within 20)
            if (W > 65535u || H > 65535u) { c->err = "render_restir: images are limited to 65535 x 65535"; return RTX_ERR_INVALID; }
            std::vector<uint8_t> mask((size_t)W * H, 0);                                      // bit 0: own pixel, bit 1: own or within the halo
            for (uint32_t k = 0; k < f.npl >> (2u * f.tile_shift); k++) {                     // the shard's tiles, by the one rule of slot_to_pixel
                uint32_t tx, ty;
                if (!shard_tile(f, k, tx, ty)) continue;
                const uint32_t x0 = tx * ts > R ? tx * ts - R : 0u, y0 = ty * ts > R ? ty * ts - R : 0u;
                const uint32_t x1 = std::min(W, (tx + 1) * ts + R), y1 = std::min(H, (ty + 1) * ts + R);
                for (uint32_t y = y0; y < y1; y++) memset(&mask[(size_t)y * W + x0], 2, x1 - x0);
            }
            for (uint32_t k = 0; k < f.npl >> (2u * f.tile_shift); k++) {
                uint32_t tx, ty;
                if (!shard_tile(f, k, tx, ty)) continue;
                for (uint32_t y = ty * ts; y < std::min(H, (ty + 1) * ts); y++) memset(&mask[(size_t)y * W + tx * ts], 3, std::min(W, (tx + 1) * ts) - tx * ts);
            }
            // 8 x 8 pixel blocks (one wave each) in Morton order: a 256-pixel chunk is a 16 x 16 px square, the 256 consecutive chunks a range of workgroups on one
            // XCD takes (rs_wg) a 256 x 256 px square — the neighbour gathers of the spatial pass stay in that XCD's L2
            const uint32_t BX = (W + 7) / 8, BY = (H + 7) / 8;
            uint32_t side = 1; while (side < std::max(BX, BY)) side <<= 1;
            std::vector<uint32_t> lown, lhalo;
            auto spread = [](uint32_t v) { v &= 0xFFFFu; v = (v | (v << 8)) & 0x00FF00FFu; v = (v | (v << 4)) & 0x0F0F0F0Fu; v = (v | (v << 2)) & 0x33333333u; v = (v | (v << 1)) & 0x55555555u; return v; };
            std::vector<std::pair<uint32_t, uint32_t>> order; order.reserve((size_t)BX * BY);
            for (uint32_t by = 0; by < BY; by++) for (uint32_t bx = 0; bx < BX; bx++) order.push_back({spread(bx) | (spread(by) << 1), bx | (by << 16)});
            std::sort(order.begin(), order.end());
            for (const auto& e : order) {
                const uint32_t bx = (e.second & 0xFFFFu) * 8u, by = (e.second >> 16) * 8u;
                for (uint32_t y = by; y < std::min(H, by + 8); y++) for (uint32_t x = bx; x < std::min(W, bx + 8); x++) {
                    const uint8_t mk = mask[(size_t)y * W + x];
                    if (mk & 1) lown.push_back(x | (y << 16));
                    if (mk & 2) lhalo.push_back(x | (y << 16));
                }
            }
            if ((r = upload(c, c->rs.d_own, lown))) return r;
            if (sharded) { if ((r = upload(c, c->rs.d_halo, lhalo))) return r; }
            c->rs.own_count = (uint32_t)lown.size(); c->rs.halo_count = sharded ? (uint32_t)lhalo.size() : 0u; memcpy(c->rs.halo_key, key, sizeof(key));
        }
        own = (const uint32_t*)c->rs.d_own.p; nown = c->rs.own_count;
        if (sharded) { halo = (const uint32_t*)c->rs.d_halo.p; nhalo = c->rs.halo_count; } else { halo = own; nhalo = nown; }
    }
    const size_t slots = rtx_pass1_slots(p->width, p->height);
    if ((r = p1_alloc(c, slots))) return r;
    HIPCHK(c, c->rs.d_last_di.ensure(slots * 40)); HIPCHK(c, c->rs.d_last_gi.ensure(slots * 40)); HIPCHK(c, c->rs.d_last_sd.ensure(slots * 60));
    if (c->opt.restir_wave && c->opt.restir_keys) { HIPCHK(c, c->rs.d_rs_key_a.ensure(slots * 32)); HIPCHK(c, c->rs.d_rs_key_b.ensure(slots * 32)); }
    if (c->rs.last_slots != slots) {
        HIPCHK(c, hipMemsetAsync(c->rs.d_last_di.p, 0, slots * 40, c->stream)); HIPCHK(c, hipMemsetAsync(c->rs.d_last_gi.p, 0, slots * 40, c->stream));
        HIPCHK(c, hipMemsetAsync(c->rs.d_last_sd.p, 0, slots * 60, c->stream));
        c->rs.last_slots = slots;
    }
    // pass 1 writes its debug estimate into a scratch image (the displayed image is pass 3's)
    DevBuf& scratch = c->rs.d_p1scratch; HIPCHK(c, scratch.ensure((size_t)p->width * p->height * 16));     // context-owned: no per-call hipMalloc / hipFree, nothing to leak on an early return
    stats_begin(c);
    struct LaneJoin { rtx_ctx* c; ~LaneJoin() { for (hipStream_t ls : c->rs.lane_stream) if (ls) (void)hipStreamSynchronize(ls); } } lane_join{c};      // no early return leaves another lane running
    HIPCHK(c, hipMemsetAsync(c->rs.d_p1cnt.p, 0, 32, c->stream));
    uint32_t* bufs[6] = {(uint32_t*)c->rs.d_res_di.p, (uint32_t*)c->rs.d_res_gi.p, (uint32_t*)c->rs.d_sdata.p, (uint32_t*)c->rs.d_last_di.p, (uint32_t*)c->rs.d_last_gi.p, (uint32_t*)c->rs.d_last_sd.p};
    if (!c->rs.hist_all) {                       // the history this context holds does not cover the image (a sharded frame came before, and no all-gather since): count reads outside it
        f.hist_x0 = c->rs.hist[0]; f.hist_y0 = c->rs.hist[1]; f.hist_x1 = c->rs.hist[2]; f.hist_y1 = c->rs.hist[3];
        f.hist_stale = (unsigned long long*)c->rs.d_p1cnt.p + 3;
    }
    const uint32_t mbk = (uint32_t)c->num_cus * 8u;
    const CameraGPU* cam = (const CameraGPU*)c->d_cam.p;
    HIPCHK(c, hipEventRecord(c->ev.begin, c->stream));
    for (uint32_t fr = 0; fr < p->spp; fr++) {                       // spp = number of consecutive frames with this camera
        DevFrame ff = f; ff.frame_seed = p->frame_seed + fr;
        HIPCHK(c, hipMemsetAsync(scratch.p, 0, (size_t)p->width * p->height * 16, c->stream));
        if (c->opt.restir_wave) {                                                                                                               // the three DispatchRays of Renderer.cpp:646-673 as wavefront stages
            if ((r = rs_lanes(c, halo, nhalo, [&](const uint32_t* px, uint32_t n, uint32_t lane, hipStream_t st) { return rs_pass1(c, ff, 1u, (F4*)scratch.p, px, n, bufs, lane, st); }))) return r;   // passes 1 + 2
            if ((r = rs_lanes(c, own, nown, [&](const uint32_t* px, uint32_t n, uint32_t lane, hipStream_t st) { return rs_pass3(c, ff, bufs, c->accum_ptr(), px, n, lane, st); }))) return r;
        } else {                                                                                                                            // ... or literally, a thread per pixel
            { Timed t(c, RTX_K_BOUNCE); launch_v6_pass1(c->stream, mbk, c->plain_scene(), ff, cam, 1u, (F4*)scratch.p, bufs[0], bufs[1], bufs[2], (unsigned long long*)c->rs.d_p1cnt.p, sharded ? halo : nullptr, sharded ? nhalo : 0u); }   // Renderer.cpp:651-654
            { Timed t(c, RTX_K_BOUNCE); launch_restir_pass2(c->stream, mbk, c->plain_scene(), ff, cam, bufs, (unsigned long long*)c->rs.d_p1cnt.p, sharded ? halo : nullptr, sharded ? nhalo : 0u); }                                       // :662-664
            { Timed t(c, RTX_K_BOUNCE); launch_restir_pass3(c->stream, mbk, c->plain_scene(), ff, cam, bufs, c->accum_ptr(), (unsigned long long*)c->rs.d_p1cnt.p); }                                    // :671-673
        }
    }
    HIPCHK(c, hipEventRecord(c->ev.end, c->stream));
    HIPCHK(c, hipGetLastError());
    unsigned long long cnt[4] = {0, 0, 0, 0};
    TO_HOST(c, cnt, c->rs.d_p1cnt.p, 32);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    stats_end_restir(c, cnt);
    c->stats.restir_stale_history_reads = cnt[3];
    // pass 3 wrote this frame's history for the pixels it ran on: the whole image, or — on shards — the own tiles (one rectangle in the block deal; the round-robin deal
    // has no rectangle to describe them: every temporal read counts as stale until rtx_restir_unpack_state has brought the other ranks' tiles)
    c->rs.hist_all = !sharded;
    if (sharded) {
        if (f.blk_gx) block_rect(p->width, p->height, f.tile_size, f.tiles_x, f.tiles_y, f.blk_gx, f.blk_gy, f.shard_rank, c->rs.hist);
        else c->rs.hist[0] = c->rs.hist[1] = c->rs.hist[2] = c->rs.hist[3] = 0;
    }
    return RTX_OK;
}

// ---- ReSTIR on shards: exchange of the history (u3 / u5 / u7) of the shard's own tiles, see rtx_render_restir ----
int rtx_restir_state_slab_bytes(const rtx_params* p, size_t* bytes) {
    if (!bytes) return RTX_ERR_INVALID;
    uint32_t ts = 0, cnt = 0; uint64_t npl = 0;
    if (const char* e = validate_tiling(p, ts, cnt, npl)) { g_create_err = e; return RTX_ERR_INVALID; }
    *bytes = (size_t)npl * 140;             // 40 + 40 + 60 bytes per local pixel slot
    return RTX_OK;
}
static int restir_state_bufs(rtx_ctx* c, const rtx_params* p, DevFrame& f, uint32_t* bufs[6]) {
    int r = make_frame(c, p, f); if (r) return r;
    const size_t slots = rtx_pass1_slots(p->width, p->height);
    if (!c->rs.last_slots || c->rs.last_slots != slots) { c->err = "restir state: no ReSTIR history of that image size (render a frame first)"; return RTX_ERR_STATE; }
    bufs[0] = (uint32_t*)c->rs.d_res_di.p; bufs[1] = (uint32_t*)c->rs.d_res_gi.p; bufs[2] = (uint32_t*)c->rs.d_sdata.p;
    bufs[3] = (uint32_t*)c->rs.d_last_di.p; bufs[4] = (uint32_t*)c->rs.d_last_gi.p; bufs[5] = (uint32_t*)c->rs.d_last_sd.p;
    return RTX_OK;
}
int rtx_restir_pack_state(rtx_ctx* c, const rtx_params* p, void* slab) {
    BIND(c);
    DevFrame f; uint32_t* bufs[6];
    int r = restir_state_bufs(c, p, f, bufs); if (r) return r;
    if (!slab) return RTX_ERR_INVALID;
    launch_restir_pack_state(c->stream, (uint32_t)c->num_cus * 8u, f, bufs, (uint32_t*)slab);
    HIPCHK(c, hipGetLastError());
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));      // on a caller-bound stream the gather that follows is stream-ordered
    return RTX_OK;
}
int rtx_restir_unpack_state(rtx_ctx* c, const rtx_params* p, const void* slabs) {
    BIND(c);
    DevFrame f; uint32_t* bufs[6];
    int r = restir_state_bufs(c, p, f, bufs); if (r) return r;
    if (!slabs) return RTX_ERR_INVALID;
    launch_restir_unpack_state(c->stream, (uint32_t)c->num_cus * 8u, f, f.shard_count, (const uint32_t*)slabs, bufs);
    HIPCHK(c, hipGetLastError());
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rs.hist_all = true;                     // every rank's tiles are here now
    return RTX_OK;
}

// ---- ... or of its border strips only (rtx.h: rtx_restir_pack_halo) ----
// Peers of rank r in the block deal: every rank q != r whose rectangle comes within halo_px of r's.  send = rect(r) ∩ dilate(rect(q)), recv = rect(q) ∩ dilate(rect(r)).
struct HaloPlan { std::vector<rtx_halo_peer> peers; uint64_t send_total = 0, recv_total = 0; uint32_t own[4] = {0, 0, 0, 0}; };
static const char* halo_plan(const rtx_params* p, uint32_t halo, HaloPlan& P) {
    uint32_t ts = 0, cnt = 0, gx = 0, gy = 0; uint64_t npl = 0;
    if (const char* e = validate_tiling(p, ts, cnt, npl, &gx, &gy)) return e;
    if (cnt < 2 || !gx) return "halo exchange: needs shard_count > 1 and RTX_FLAG_BLOCK_TILES (one rectangle of tiles per rank)";
    if (halo == 0 || halo > 4096) return "halo exchange: halo_px must be in [1, 4096]";
    const uint32_t W = p->width, H = p->height, TX = (W + ts - 1) / ts, TY = (H + ts - 1) / ts;
    block_rect(W, H, ts, TX, TY, gx, gy, p->shard_rank, P.own);
    auto clip = [](const uint32_t a[4], const uint32_t b[4], uint32_t grow, uint32_t W_, uint32_t H_, uint32_t out[4]) {      // a ∩ dilate(b, grow); false: empty
        const uint32_t bx0 = b[0] > grow ? b[0] - grow : 0u, by0 = b[1] > grow ? b[1] - grow : 0u, bx1 = std::min(W_, b[2] + grow), by1 = std::min(H_, b[3] + grow);
        out[0] = std::max(a[0], bx0); out[1] = std::max(a[1], by0); out[2] = std::min(a[2], bx1); out[3] = std::min(a[3], by1);
        return out[0] < out[2] && out[1] < out[3];
    };
    P.peers.clear(); P.send_total = P.recv_total = 0;
    if (P.own[0] >= P.own[2] || P.own[1] >= P.own[3]) return nullptr;                          // a rank without pixels (more ranks than tile columns): no peers
    for (uint32_t q = 0; q < cnt; q++) {
        if (q == p->shard_rank) continue;
        uint32_t rq[4], sr[4], rr[4]; block_rect(W, H, ts, TX, TY, gx, gy, q, rq);
        if (rq[0] >= rq[2] || rq[1] >= rq[3]) continue;
        if (!clip(P.own, rq, halo, W, H, sr) || !clip(rq, P.own, halo, W, H, rr)) continue;         // (both are empty or neither is: the dilation is symmetric)
        rtx_halo_peer e{}; e.rank = q;
        e.send_x0 = sr[0]; e.send_y0 = sr[1]; e.send_x1 = sr[2]; e.send_y1 = sr[3]; e.recv_x0 = rr[0]; e.recv_y0 = rr[1]; e.recv_x1 = rr[2]; e.recv_y1 = rr[3];
        e.send_offset = P.send_total; e.send_bytes = (uint64_t)(sr[2] - sr[0]) * (sr[3] - sr[1]) * 140u; P.send_total += e.send_bytes;
        e.recv_offset = P.recv_total; e.recv_bytes = (uint64_t)(rr[2] - rr[0]) * (rr[3] - rr[1]) * 140u; P.recv_total += e.recv_bytes;
        P.peers.push_back(e);
    }
    if (P.send_total / 140u > 0xFFFFFFFFull || P.recv_total / 140u > 0xFFFFFFFFull) return "halo exchange: regions too large";
    return nullptr;
}
int rtx_restir_halo_plan(const rtx_params* p, uint32_t halo_px, rtx_halo_peer* peers, uint32_t max_peers, uint32_t* npeers, uint64_t* send_total, uint64_t* recv_total) {
    HaloPlan P;
    if (const char* e = halo_plan(p, halo_px, P)) { g_create_err = e; return RTX_ERR_INVALID; }
    if (npeers) *npeers = (uint32_t)P.peers.size();
    if (send_total) *send_total = P.send_total;
    if (recv_total) *recv_total = P.recv_total;
    if (peers) {
        if (P.peers.size() > max_peers) { g_create_err = "halo plan: more peers than the caller's array holds"; return RTX_ERR_INVALID; }
        for (size_t i = 0; i < P.peers.size(); i++) peers[i] = P.peers[i];
    }
    return RTX_OK;
}
static int halo_move(rtx_ctx* c, const rtx_params* p, uint32_t halo_px, void* buf, bool pack) {
    DevFrame f; uint32_t* bufs[6];
    int r = restir_state_bufs(c, p, f, bufs); if (r) return r;
    HaloPlan P;
    if (const char* e = halo_plan(p, halo_px, P)) { c->err = e; return RTX_ERR_INVALID; }
    if (!buf && (pack ? P.send_total : P.recv_total)) return RTX_ERR_INVALID;
    for (size_t i = 0; i < P.peers.size(); i += kHaloPeers) {                                  // (<= 8 peers in practice: one launch)
        uint32_t rects[4 * kHaloPeers]; uint32_t n = 0;
        for (; n < kHaloPeers && i + n < P.peers.size(); n++) {
            const rtx_halo_peer& e = P.peers[i + n];
            rects[4 * n] = pack ? e.send_x0 : e.recv_x0; rects[4 * n + 1] = pack ? e.send_y0 : e.recv_y0;
            rects[4 * n + 2] = pack ? e.send_x1 - e.send_x0 : e.recv_x1 - e.recv_x0; rects[4 * n + 3] = pack ? e.send_y1 - e.send_y0 : e.recv_y1 - e.recv_y0;
        }
        const uint64_t off = pack ? P.peers[i].send_offset : P.peers[i].recv_offset;
        launch_restir_halo(c->stream, (uint32_t)c->num_cus * 8u, p->width, pack, rects, n, bufs, (uint32_t*)((char*)buf + off));
    }
    HIPCHK(c, hipGetLastError());
    if (c->own_stream) HIPCHK(c, hipStreamSynchronize(c->stream));      // on a caller-bound stream the exchange that follows is stream-ordered
    if (!pack) {                                                        // the history now covers my rectangle + the halo (clipped to the image)
        c->rs.hist_all = false;
        c->rs.hist[0] = P.own[0] > halo_px ? P.own[0] - halo_px : 0u; c->rs.hist[1] = P.own[1] > halo_px ? P.own[1] - halo_px : 0u;
        c->rs.hist[2] = std::min(p->width, P.own[2] + halo_px); c->rs.hist[3] = std::min(p->height, P.own[3] + halo_px);
    }
    return RTX_OK;
}
int rtx_restir_pack_halo(rtx_ctx* c, const rtx_params* p, uint32_t halo_px, void* send) { BIND(c); return halo_move(c, p, halo_px, send, true); }
int rtx_restir_unpack_halo(rtx_ctx* c, const rtx_params* p, uint32_t halo_px, const void* recv) { BIND(c); return halo_move(c, p, halo_px, const_cast<void*>(recv), false); }

int rtx_read_restir_last(rtx_ctx* c, void* di, void* gi, void* sd, size_t slots) {
    BIND(c);
    if (!c->rs.last_slots || slots < c->rs.last_slots) { c->err = "read_restir_last: no ReSTIR state or too few slots"; return RTX_ERR_INVALID; }
    if (di) TO_HOST(c, di, c->rs.d_last_di.p, c->rs.last_slots * 40);
    if (gi) TO_HOST(c, gi, c->rs.d_last_gi.p, c->rs.last_slots * 40);
    if (sd) TO_HOST(c, sd, c->rs.d_last_sd.p, c->rs.last_slots * 60);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

int rtx_read_pass1_buffers(rtx_ctx* c, void* di, void* gi, void* sd, size_t slots) {
    BIND(c);
    if (!c->rs.p1_slots || slots < c->rs.p1_slots) { c->err = "read_pass1_buffers: no pass-1 data or too few slots"; return RTX_ERR_INVALID; }
    if (di) TO_HOST(c, di, c->rs.d_res_di.p, c->rs.p1_slots * 40);
    if (gi) TO_HOST(c, gi, c->rs.d_res_gi.p, c->rs.p1_slots * 40);
    if (sd) TO_HOST(c, sd, c->rs.d_sdata.p, c->rs.p1_slots * 60);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RTX_OK;
}

}  // extern "C"

// rtx_kernels.hip — the wavefront path-tracing kernels for gfx950 (CDNA4, wave64): the map of the design, the kernel headers (rtx_k_*.hpp, rtx_restir*.hpp) and their launchers.
//
// One sample batch is a set of paths with fixed slots ("pid"); per-path state lives in SoA float4 arrays in HBM.
// General scenes: each bounce runs  k_trace_closest -> k_shade -> k_trace_shadow[j]  over workgroup-private index
// sub-queues that k_shade re-compacts with a wave ballot + prefix sum (one LDS atomic per wave, no global atomics);
// the traversal kernels are persistent waves with dynamic ray fetch, the top of the BVH and the per-lane stack live
// in LDS.  Tiny scenes (<= 64 triangles, the Cornell Box): no BVH, a packed-FP32 plane/edge pre-test with
// scalar-loaded coefficients, and ONE fused kernel per bounce (k_bounce_small).  The reference's own passes
// (k_v6_pass1, k_restir_pass2/3) are thread-per-pixel kernels.  MFMA is unused on purpose: nothing here is a dense
// contraction.
//
// Parity-critical arithmetic (ray/triangle test, surface reconstruction, BSDF, light sampling, path
// throughput) follows rtx_math.hpp / rtx_bsdf.hpp with the library-wide -ffp-contract=off.  Ray/box
// tests are NOT parity-critical (closest hit is defined as the minimum over all triangles with a
// lowest-id tie break, any-hit as existence), they only have to be conservative.
//
// ONE translation unit, the kernels in headers by concern: the tooling builds' device globals (g_sec and g_trv with PROFILE=1, g_wgt with -DRTX_WAVE_CLOCK) are written by the trace,
// shade and fused kernels and read by the rtx_debug_* entry points at the end of this file, and without relocatable device code a global cannot cross translation units.
// The commit path's kernels (refit, tree cost) need none of this: rtx_refit.hip.
#include <hip/hip_runtime.h>
#include <type_traits>
#include "rtx_kernels.hpp"
#include "rtx_dev_common.hpp"   // wave helpers, compaction, slot -> pixel, primary ray
#include "rtx_traverse.hpp"     // triangle test, 8-wide BVH traversal (simple + persistent), tiny-scene pre-test
#include "rtx_shade.hpp"        // surface reconstruction, NEE, BSDF continuation
#include "rtx_restir.hpp"       // k_v6_pass1, k_restir_pass2 / 3 (thread per pixel) + the shared per-pixel math
#include "rtx_restir_wave.hpp"  // the same three passes as wavefront stages

namespace rtx {

#ifdef RTX_PROFILE_SECTIONS
__device__ unsigned long long g_sec[36];          // [0,12) cycles, [12,24) active lanes summed, [24,36) calls
#define PF_BEGIN Prof pfv; pfv.begin(); Prof* pf = &pfv
#define PF_MARK(i) pf->mark(i)
#define PF_COUNT(i) pf->count(i)
#define PF_FLUSH do { if (lane_id() == 0) for (int i = 0; i < 12; i++) { atomicAdd(&g_sec[i], pfv.acc[i]); atomicAdd(&g_sec[12 + i], pfv.lanes[i]); atomicAdd(&g_sec[24 + i], pfv.calls[i]); } } while (0)
#else
#define PF_BEGIN Prof* pf = nullptr; (void)pf
#define PF_MARK(i) do { } while (0)
#define PF_COUNT(i) do { } while (0)
#define PF_FLUSH do { } while (0)
#endif

}  // namespace rtx

// the kernels, by concern
#include "rtx_k_raygen.hpp"         // k_raygen, k_packet_masks, k_raygen_trace_small, k_primary_surface, k_raygen_shared (the pixel -> ray step of the first and third: camera_sample, rtx_dev_common.hpp)
#include "rtx_k_trace.hpp"          // k_trace_closest, k_trace_shadow
#include "rtx_k_shade.hpp"          // k_shade, k_shade_dense
#include "rtx_k_bounce_small.hpp"   // k_bounce_small
#include "rtx_k_bounce_bvh.hpp"     // k_bounce_bvh, k_order_queues
#include "rtx_k_film.hpp"           // k_accumulate, k_srgb8, k_debug_layer, k_pack_tiles, k_unpack_tiles
#include "rtx_k_adaptive.hpp"       // k_adaptive_error, k_adaptive_compact
#include "rtx_k_denoise.hpp"        // k_denoise_guides, k_denoise_level (both filters), k_denoise_var_input, k_denoise_count
#include "rtx_k_dbg.hpp"            // k_dbg_*

namespace rtx {

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
static inline uint32_t grid_for(uint32_t items, uint32_t max_blocks) {
    uint32_t b = (items + kBlock - 1) / kBlock;
    if (b < 1) b = 1;
    return b < max_blocks ? b : max_blocks;
}
static inline size_t small_planes_bytes(const DevScene& sc) { return sc.nsmall ? (size_t)small_planes_count(sc.nsmall) * 16 : 0; }   // stage_lds
size_t trace_lds_bytes(const DevScene& sc) {      // the LDS column stack is always reserved: debug / pass-1 kernels use it
    return (size_t)sc.lds_nodes * 80 + (size_t)sc.lds_tris * 48 + small_planes_bytes(sc) + (size_t)sc.stack_depth * kBlock * kStackEntryBytes;
}
size_t trace_lds_bytes_queue(const DevScene& sc) {   // queue kernels with a private stack need no LDS stack
    const size_t stack = sc.stack_private == 1 ? 0 : (size_t)sc.stack_depth * kBlock * kStackEntryBytes;
    return (size_t)sc.lds_nodes * 80 + (size_t)sc.lds_tris * 48 + small_planes_bytes(sc) + stack;
}

// workgroups of the two persistent traversal kernels (default instantiations; their CUT forms when the scene launches those) that fit on a CU with this scene's LDS layout; 0 = query failed
int trace_workgroups_per_cu(const DevScene& sc) {
    int a = 0, b = 0;
    if (sc.tri_cut) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_trace_closest<0, false, 6, true>, (int)kBlock, trace_lds_bytes(sc)) != hipSuccess) return 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_trace_shadow<0, false, 6, 0, true>, (int)kBlock, trace_lds_bytes(sc)) != hipSuccess) return 0;
        return a < b ? a : b;
    }
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_trace_closest<0, false, 6>, (int)kBlock, trace_lds_bytes(sc)) != hipSuccess) return 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_trace_shadow<0, false, 6>, (int)kBlock, trace_lds_bytes(sc)) != hipSuccess) return 0;
    return a < b ? a : b;
}
// run-time choices as compile-time constants: a launcher names its kernel once, with template arguments taken from the types of std::integral_constants
template <int V> using IntC = std::integral_constant<int, V>;
template <bool V> using BoolC = std::integral_constant<bool, V>;
template <class F> static void dispatch_bool(bool v, F f) { if (v) f(BoolC<true>{}); else f(BoolC<false>{}); }

void launch_raygen(hipStream_t st, const DevFrame& f, const DevPaths& p, const CameraGPU* cam, uint32_t* queue, uint32_t* qcount, bool compact) {
    dispatch_bool(f.list != nullptr, [&](auto list) { dispatch_bool(f.lens_radius > 0.0f, [&](auto lens) {
        hipLaunchKernelGGL((k_raygen<decltype(list)::value, decltype(lens)::value>), dim3(f.nblocks), dim3(kBlock), 0, st, f, p, cam, queue, qcount, compact ? 1u : 0u);
    }); });
}
void launch_packet_masks(hipStream_t st, const DevScene& sc, const DevFrame& f, const CameraGPU* cam, unsigned long long* masks) {
    const uint32_t nblk = f.npl / 64u;
    hipLaunchKernelGGL(k_packet_masks, dim3((nblk + 3u) / 4u), dim3(kBlock), 0, st, sc, f, cam, masks);
}
void launch_raygen_trace_small(hipStream_t st, const DevScene& sc, const DevFrame& f, const DevPaths& p, const CameraGPU* cam, uint32_t* queue, uint32_t* qcount, uint32_t* gencount, const unsigned long long* masks) {
    dispatch_bool(f.list != nullptr, [&](auto list) { dispatch_bool(f.lens_radius > 0.0f, [&](auto lens) {
        hipLaunchKernelGGL((k_raygen_trace_small<decltype(list)::value, decltype(lens)::value>), dim3(f.nblocks), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, f, p, cam, queue, qcount, gencount, masks);
    }); });
}
void launch_primary_surface(hipStream_t st, const DevScene& sc, const DevFrame& f, const CameraGPU* cam, unsigned long long* masks, unsigned long long* hits, F4* rec) {
    hipLaunchKernelGGL(k_primary_surface, dim3(f.npl / kBlock), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, f, cam, masks, hits, rec);
}
void launch_raygen_shared(hipStream_t st, const DevFrame& f, uint32_t* queue, uint32_t* qcount, uint32_t* gencount, const unsigned long long* hits, uint32_t rec_npl) {
    dispatch_bool(f.list != nullptr, [&](auto list) { hipLaunchKernelGGL(k_raygen_shared<decltype(list)::value>, dim3(f.nblocks), dim3(kBlock), 0, st, f, queue, qcount, gencount, hits, rec_npl >> 6); });
}
// The launch of a persistent traversal kernel (k_trace_closest, k_trace_shadow): clamps `merge`, sizes the grid and maps (sc, heads) to the instantiation — stack kind, stealing,
// compiled-in schedule, as std::integral_constants (IntC / BoolC above) — and its dynamic LDS.  launch(stk, steal, sched, grid, lds_bytes, heads, merge) does the launch.
// (launch_trace_occ has a narrower choice of its own: no private stack, no stealing.  Through this helper it would instantiate SINK-1 kernels nobody launches.)
// A scene with a cut-out triangle (sc.tri_cut) never steals, so that the callers' CUT instantiations exist for the other five combinations only (with_cut below).
template <class Launch>
static void launch_trace_variant(const DevFrame& f, const DevScene& sc, uint32_t* heads, uint32_t merge, Launch launch) {
    if (sc.nsmall || sc.tri_cut) heads = nullptr;                     // (the un-fused tiny-scene test path has no persistent waves)
    if (heads || sc.nsmall || merge < 1u) merge = 1u;
    if (merge > kMaxMerge) merge = kMaxMerge;
    const uint32_t grid = (f.nblocks + merge - 1u) / merge;
    const bool sched6 = sc.trace_sched == 6u && !sc.nsmall && !sc.trace_cnt;      // the default configuration: schedule compiled in (the work counters live in the generic instantiation)
    auto go = [&](auto stk, auto steal, auto sched, size_t lds_bytes) { launch(stk, steal, sched, grid, lds_bytes, heads, merge); };
    if (sc.stack_private == 1) { if (heads) go(IntC<1>{}, BoolC<true>{}, IntC<-1>{}, trace_lds_bytes_queue(sc)); else go(IntC<1>{}, BoolC<false>{}, IntC<-1>{}, trace_lds_bytes_queue(sc)); }
    else if (sc.stack_ovf) {                                // RTX_OPT_STACK_CAP: the tree needs more entries than the LDS column holds (StackLdsT<true>)
        if (heads) go(IntC<2>{}, BoolC<true>{}, IntC<-1>{}, trace_lds_bytes(sc));
        else if (sched6) go(IntC<2>{}, BoolC<false>{}, IntC<6>{}, trace_lds_bytes(sc));
        else go(IntC<2>{}, BoolC<false>{}, IntC<-1>{}, trace_lds_bytes(sc));
    }
    else if (heads) go(IntC<0>{}, BoolC<true>{}, IntC<-1>{}, trace_lds_bytes(sc));
#ifndef RTX_NO_SCHED_SPECIAL
    else if (sched6) go(IntC<0>{}, BoolC<false>{}, IntC<6>{}, trace_lds_bytes(sc));
#endif
    else go(IntC<0>{}, BoolC<false>{}, IntC<-1>{}, trace_lds_bytes(sc));
}
// the CUT argument of a traversal launch: go(BoolC<sc.tri_cut != nullptr>) — except for the stealing combinations, which have no CUT instantiation (and are never chosen with cut-outs)
template <bool STEAL, class Go> static void with_cut(const DevScene& sc, Go go) {
    if constexpr (STEAL) go(BoolC<false>{}); else dispatch_bool(sc.tri_cut != nullptr, go);
}
void launch_trace_closest(hipStream_t st, const DevFrame& f, const DevScene& sc, const DevPaths& p, uint32_t bounce, const uint32_t* queue, const uint32_t* qcount, uint32_t* heads, uint32_t merge) {
    const float tmin = bounce == 0 ? kTMinCam : kSBias;
    launch_trace_variant(f, sc, heads, merge, [&](auto stk, auto steal, auto sched, uint32_t grid, size_t lds_bytes, uint32_t* hd, uint32_t mg) {
        with_cut<decltype(steal)::value>(sc, [&](auto cut) {
            hipLaunchKernelGGL((k_trace_closest<decltype(stk)::value, decltype(steal)::value, decltype(sched)::value, decltype(cut)::value>), dim3(grid), dim3(kBlock), lds_bytes, st,
                               sc, sc.small, p, queue, qcount, f.qcap, tmin, sc.refill_min, sc.trace_sched, hd, f.nblocks, mg);
        });
    });
}
void launch_bounce_small(hipStream_t st, const DevScene& sc, const DevFrame& f, const DevPaths& p, uint32_t bounce_first, uint32_t bounce_end,
                         uint32_t* queue_a, uint32_t* queue_b, uint32_t* qrows, uint32_t* srows, const uint32_t* order, int variant, const PrimIn* prim) {
    // general instantiation: 118 VGPRs, 4 waves/SIMD (5 or 6 spill and measured slower); Lambert-only: 85 VGPRs, 5 waves/SIMD (a build for 6 waves, 80 VGPRs
    // with 2 spilled, measured the same: 19.13 vs 19.03 ms).  Bounce 0 (reads the primary hits) is its own instantiation and launch.
    const bool lam = (f.flags & 1u) != 0u, have_hit = bounce_first == 0u;
    const PrimIn pin = prim ? *prim : PrimIn{};
    // cc: the path state by queue position in two sets (p.out_o != nullptr, RTX_OPT_COMPACT_STATE).  The block-scheduled forms of bounces >= 1 have no such instantiation:
    // the host plans a frame that runs one of them in place (plan_batches), and DevPaths says so
    auto go = [&](auto hh, auto rr, auto cc) {       // hh: where bounce 0's hits come from (0 = not bounce 0, 1 = the hit buffer, 2 = the shared primary records); rr: RING — the form of bounces >= 1 (RTX_OPT_BOUNCE_VARIANT 0 / 1 / 2 = RING 1 / 0 / 2)
        dispatch_bool(lam, [&](auto ll) {
            hipLaunchKernelGGL((k_bounce_small<4, decltype(hh)::value, decltype(ll)::value, decltype(rr)::value, decltype(cc)::value>), dim3(f.nblocks), dim3(kBlock), trace_lds_bytes(sc), st,
                               sc, sc.small, f, p, bounce_first, bounce_end, queue_a, queue_b, qrows, srows, order, pin);
        });
    };
    const bool compact = p.out_o != nullptr;
    if (have_hit && prim) dispatch_bool(compact, [&](auto cc) { go(IntC<2>{}, IntC<0>{}, cc); });
    else if (have_hit) dispatch_bool(compact, [&](auto cc) { go(IntC<1>{}, IntC<0>{}, cc); });
    else if (variant == 2) dispatch_bool(compact, [&](auto cc) { go(IntC<0>{}, IntC<2>{}, cc); });
    else if (variant == 1) go(IntC<0>{}, IntC<0>{}, BoolC<false>{});
    else go(IntC<0>{}, IntC<1>{}, BoolC<false>{});
}
void launch_bounce_bvh(hipStream_t st, const DevScene& sc, const DevFrame& f, const DevPaths& p, uint32_t bounce_first, uint32_t bounce_end,
                       uint32_t* queue_a, uint32_t* queue_b, uint32_t* hitq, uint32_t* qrows, uint32_t* srows, const uint32_t* order) {
    if (sc.stack_private == 1) hipLaunchKernelGGL(k_bounce_bvh<1>, dim3(f.nblocks), dim3(kBlock), trace_lds_bytes_queue(sc), st, sc, f, p, bounce_first, bounce_end, queue_a, queue_b, hitq, qrows, srows, order);
    else if (sc.stack_ovf) hipLaunchKernelGGL(k_bounce_bvh<2>, dim3(f.nblocks), dim3(kBlock), trace_lds_bytes(sc), st, sc, f, p, bounce_first, bounce_end, queue_a, queue_b, hitq, qrows, srows, order);
    else hipLaunchKernelGGL(k_bounce_bvh<0>, dim3(f.nblocks), dim3(kBlock), trace_lds_bytes(sc), st, sc, f, p, bounce_first, bounce_end, queue_a, queue_b, hitq, qrows, srows, order);
}
void launch_order_queues(hipStream_t st, const uint32_t* qcount, uint32_t G, uint32_t* order) {
    hipLaunchKernelGGL(k_order_queues, dim3(1), dim3(1024), 0, st, qcount, G, order);
}
void launch_trace_shadow(hipStream_t st, const DevFrame& f, const DevScene& sc, const DevPaths& p, uint32_t j, const uint32_t* shcount, uint32_t* heads, uint32_t merge) {
    const size_t seg = (size_t)j * f.qcap * f.nblocks;
    launch_trace_variant(f, sc, heads, merge, [&](auto stk, auto steal, auto sched, uint32_t grid, size_t lds_bytes, uint32_t* hd, uint32_t mg) {
        with_cut<decltype(steal)::value>(sc, [&](auto cut) {
            hipLaunchKernelGGL((k_trace_shadow<decltype(stk)::value, decltype(steal)::value, decltype(sched)::value, 0, decltype(cut)::value>), dim3(grid), dim3(kBlock), lds_bytes, st,
                               sc, sc.small, p, p.sh_o + seg, p.sh_d + seg, p.sh_c + seg, shcount, f.qcap, sc.refill_min, sc.trace_sched, hd, f.nblocks, mg);
        });
    });
}
static size_t shade_lds_bytes(const DevScene& sc, bool sort) { uint32_t lb, mb; shade_lds_plan(sc.nlights, sc.nmat, sort, lb, mb); return (size_t)lb + mb; }
void launch_shade(hipStream_t st, const DevScene& sc, const DevFrame& f, const DevPaths& p, uint32_t bounce,
                  const uint32_t* queue, const uint32_t* qcount, uint32_t* next_queue, uint32_t* next_count, uint32_t* shcounts) {
    // material-sorted variant: measured slower (see k_shade), the permutation un-coalesces the per-path state streams
    dispatch_bool((f.flags & 1u) != 0u, [&](auto lam) {
        constexpr bool LL = decltype(lam)::value;
        // a texture map is active: the default kernel's TEX form, whatever RTX_OPT_SHADE_DENSE / RTX_OPT_SORT_MATERIALS say (the rejected variants get no textured copy)
        // an environment is bound: the default kernel too, in its ENV form when the map has weight (a black map adds nothing and casts nothing: the kernels without it)
        // a specular map is active and the frame is not RTX_FLAG_LAMBERT_ONLY: the SPC form of the TEX kernel (tri_uv is set whenever map_pr is), with or without the
        // environment's sample and the normal maps.  A Lambert-only frame reads none of the three: it falls through to the kernels below
        // an emission map is active: the EMI form of the TEX kernel (tri_uv is set whenever map_ke is), Lambert or GGX, with or without the environment's sample, the normal maps
        // (tri_tan exists only while one is active) and, in a GGX frame, the specular maps
        if (sc.map_ke) {
            uint32_t lb, mb; shade_lds_plan(sc.nlights, sc.nmat, false, lb, mb);
            dispatch_bool(sc.env_tex != nullptr, [&](auto env) { dispatch_bool(sc.tri_tan != nullptr, [&](auto nrm) { dispatch_bool(!LL && sc.map_pr != nullptr, [&](auto spc) {
                constexpr bool EE = decltype(env)::value, SS = !LL && decltype(spc)::value;
                hipLaunchKernelGGL((k_shade<false, LL, true, EE, decltype(nrm)::value, SS, true>), dim3(f.nblocks), dim3(kBlock), (size_t)lb + mb + (EE ? shade_env_lds(lb, mb, sc.env_n) : 0u), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
            }); }); });
            return;
        }
        if constexpr (!LL) if (sc.map_pr) {
            uint32_t lb, mb; shade_lds_plan(sc.nlights, sc.nmat, false, lb, mb);
            dispatch_bool(sc.env_tex != nullptr, [&](auto env) { dispatch_bool(sc.tri_tan != nullptr, [&](auto nrm) {
                constexpr bool EE = decltype(env)::value;
                hipLaunchKernelGGL((k_shade<false, false, true, EE, decltype(nrm)::value, true>), dim3(f.nblocks), dim3(kBlock), (size_t)lb + mb + (EE ? shade_env_lds(lb, mb, sc.env_n) : 0u), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
            }); });
            return;
        }
        if (sc.env_n) {
            uint32_t lb, mb; shade_lds_plan(sc.nlights, sc.nmat, false, lb, mb);
            // a normal map is active: the NRM form of the TEX kernel (tri_uv is set whenever tri_tan is), with or without the environment's sample
            if (sc.tri_tan) {
                dispatch_bool(sc.env_tex != nullptr, [&](auto env) {
                    constexpr bool EE = decltype(env)::value;
                    hipLaunchKernelGGL((k_shade<false, LL, true, EE, true>), dim3(f.nblocks), dim3(kBlock), (size_t)lb + mb + (EE ? shade_env_lds(lb, mb, sc.env_n) : 0u), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
                });
                return;
            }
            dispatch_bool(sc.tri_uv != nullptr, [&](auto tex) { dispatch_bool(sc.env_tex != nullptr, [&](auto env) {
                constexpr bool EE = decltype(env)::value;
                hipLaunchKernelGGL((k_shade<false, LL, decltype(tex)::value, EE>), dim3(f.nblocks), dim3(kBlock), (size_t)lb + mb + (EE ? shade_env_lds(lb, mb, sc.env_n) : 0u), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
            }); });
            return;
        }
        if (sc.tri_tan) { hipLaunchKernelGGL((k_shade<false, LL, true, false, true>), dim3(f.nblocks), dim3(kBlock), shade_lds_bytes(sc, false), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts); return; }
        if (sc.tri_uv) { hipLaunchKernelGGL((k_shade<false, LL, true>), dim3(f.nblocks), dim3(kBlock), shade_lds_bytes(sc, false), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts); return; }
        if (sc.shade_dense && !sc.sort_materials) hipLaunchKernelGGL((k_shade_dense<LL>), dim3(f.nblocks), dim3(kBlock), 0, st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
        else dispatch_bool(sc.sort_materials != 0u, [&](auto sort) {
            constexpr bool SS = decltype(sort)::value;
            hipLaunchKernelGGL((k_shade<SS, LL>), dim3(f.nblocks), dim3(kBlock), shade_lds_bytes(sc, SS), st, sc, f, p, bounce, queue, qcount, next_queue, next_count, shcounts);
        });
    });
}
void launch_v6_pass1(hipStream_t st, uint32_t max_blocks, const DevScene& sc, const DevFrame& f, const CameraGPU* cam, uint32_t sample_id,
                     F4* accum, uint32_t* res_di, uint32_t* res_gi, uint32_t* sdata, unsigned long long* counters, const uint32_t* pixels, uint32_t npixels) {
    hipLaunchKernelGGL(k_v6_pass1, dim3(grid_for(pixels ? npixels : f.npl, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, f, cam, sample_id, accum, res_di, res_gi, sdata, counters, pixels, npixels);
}
static inline RestirBufs rs_bufs(uint32_t* const* b) { return RestirBufs{b[0], b[1], b[2], b[3], b[4], b[5]}; }
void launch_restir_pass2(hipStream_t st, uint32_t max_blocks, const DevScene& sc, const DevFrame& f, const CameraGPU* cam, uint32_t* const bufs[6], unsigned long long* counters,
                         const uint32_t* pixels, uint32_t npixels) {
    hipLaunchKernelGGL(k_restir_pass2, dim3(grid_for(pixels ? npixels : f.npl, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, f, cam, rs_bufs(bufs), counters, pixels, npixels);
}
void launch_restir_pack_state(hipStream_t st, uint32_t max_blocks, const DevFrame& f, uint32_t* const bufs[6], uint32_t* slab) {
    hipLaunchKernelGGL(k_restir_pack_state, dim3(grid_for(f.npl, max_blocks)), dim3(kBlock), 0, st, f, rs_bufs(bufs), slab);
}
void launch_restir_unpack_state(hipStream_t st, uint32_t max_blocks, const DevFrame& f, uint32_t nshards, const uint32_t* slabs, uint32_t* const bufs[6]) {
    hipLaunchKernelGGL(k_restir_unpack_state, dim3(grid_for(f.npl * nshards, max_blocks)), dim3(kBlock), 0, st, f, nshards, slabs, rs_bufs(bufs));
}
// history records of n <= 16 pixel rectangles <-> one buffer (rtx_restir_pack_halo / unpack_halo): rect k = (x0, y0, w, h), records of all rectangles back to back
void launch_restir_halo(hipStream_t st, uint32_t max_blocks, uint32_t width, bool pack, const uint32_t* rects4, uint32_t n, uint32_t* const bufs[6], uint32_t* buf) {
    HaloRects R{}; R.n = n; R.first[0] = 0;
    for (uint32_t k = 0; k < n; k++) { R.x0[k] = rects4[4 * k]; R.y0[k] = rects4[4 * k + 1]; R.w[k] = rects4[4 * k + 2]; R.first[k + 1] = R.first[k] + rects4[4 * k + 2] * rects4[4 * k + 3]; }
    if (!R.first[n]) return;
    dispatch_bool(pack, [&](auto pk) { hipLaunchKernelGGL(k_restir_halo<decltype(pk)::value>, dim3(grid_for(R.first[n], max_blocks)), dim3(kBlock), 0, st, width, R, rs_bufs(bufs), buf); });
}
void launch_restir_pass3(hipStream_t st, uint32_t max_blocks, const DevScene& sc, const DevFrame& f, const CameraGPU* cam, uint32_t* const bufs[6], F4* accum, unsigned long long* counters) {
    hipLaunchKernelGGL(k_restir_pass3, dim3(grid_for(f.npl, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, f, cam, rs_bufs(bufs), accum, counters);
}
// ---- wavefront ReSTIR stages ----
void launch_trace_occ(hipStream_t st, const DevScene& sc_in, const RsQ& q, const uint32_t* shcnt) {
    DevPaths none{};
    // the visibility rays of the ReSTIR stages run between arbitrary scene points (reconnections, last frame's samples), not towards sampled lights: the NEE probe's
    // order does not carry over — slot order measured best on all three scenes (atrium 8.28 vs 8.38 ms, garage 6.74 vs 6.84, street 7.99 vs 8.02-8.12 per frame with orders 1 / 2)
    DevScene sc = sc_in; sc.any_order = sc_in.any_order_occ;
    const bool sched6 = sc.trace_sched == 6u && !sc.nsmall && !sc.trace_cnt;        // as launch_trace_variant: the default schedule compiled in
    dispatch_bool(sc.stack_ovf != nullptr, [&](auto ovf) {
        dispatch_bool(sched6, [&](auto s6) {
            hipLaunchKernelGGL((k_trace_shadow<(decltype(ovf)::value ? 2 : 0), false, (decltype(s6)::value ? 6 : -1), 1>), dim3(q.G), dim3(kBlock), trace_lds_bytes(sc), st,
                               sc, sc.small, none, q.sh_o, q.sh_d, (const F4*)nullptr, shcnt, q.rcap, sc.refill_min, sc.trace_sched, (uint32_t*)nullptr, q.G, 1u, q.sh_pay, q.occ);
        });
    });
}
void launch_rs_raygen(hipStream_t st, const DevFrame& f, const RsQ& q, const CameraGPU* cam, uint32_t sample_id, uint32_t* cnt_out) {
    hipLaunchKernelGGL(k_rs_raygen, dim3(q.G), dim3(kBlock), 0, st, f, q, cam, sample_id, cnt_out);
}
void launch_rs_p1_ris(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, const uint32_t* cnt_in, uint32_t* cnt_out, F4* accum, uint32_t* res_di, uint32_t* res_gi, uint32_t* sdata) {
    hipLaunchKernelGGL(k_rs_p1_ris, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cnt_in, cnt_out, accum, res_di, res_gi, sdata);
}
void launch_rs_p1_ris_finish(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, const uint32_t* cnt_in, uint32_t* cnt_out, uint32_t* shcnt, uint32_t* res_di, uint32_t* sdata) {
    hipLaunchKernelGGL(k_rs_p1_ris_finish, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cnt_in, cnt_out, shcnt, res_di, sdata);
}
void launch_rs_p1_first(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, const uint32_t* cnt_in, uint32_t* cnt_out) {
    hipLaunchKernelGGL(k_rs_p1_first, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cnt_in, cnt_out);
}
void launch_rs_p1_loop(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, uint32_t set, uint32_t iter, const uint32_t* cnt_in, uint32_t* cnt_out) {
    hipLaunchKernelGGL(k_rs_p1_loop, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, set, iter, cnt_in, cnt_out);
}
void launch_rs_p1_emit_final(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, const CameraGPU* cam, uint32_t* const* bufs, uint32_t* shcnt) {
    hipLaunchKernelGGL(k_rs_p1_emit_final, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cam, bufs ? rs_bufs(bufs) : RestirBufs{}, bufs ? 1u : 0u, shcnt);
}
void launch_rs_p1_finish(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, F4* accum, uint32_t* res_di, uint32_t* res_gi, uint32_t* sdata, const CameraGPU* cam, uint32_t* const* bufs) {
#ifdef RTX_RS_FUSED_FINISH       // (A/B build: make VARIANT=ffin VARFLAGS=-DRTX_RS_FUSED_FINISH — the round-3 form, both halves in one kernel)
    hipLaunchKernelGGL((k_rs_p1_finish<true, true>), dim3(q.G), dim3(kBlock), 0, st, sc, f, q, accum, res_di, res_gi, sdata, cam, bufs ? rs_bufs(bufs) : RestirBufs{}, bufs ? 1u : 0u);
#else
    hipLaunchKernelGGL((k_rs_p1_finish<true, false>), dim3(q.G), dim3(kBlock), 0, st, sc, f, q, accum, res_di, res_gi, sdata, cam, RestirBufs{}, 0u);
    if (bufs) hipLaunchKernelGGL((k_rs_p1_finish<false, true>), dim3(q.G), dim3(kBlock), 0, st, sc, f, q, accum, res_di, res_gi, sdata, cam, rs_bufs(bufs), 1u);
#endif
}
void launch_rs_p3_keys(hipStream_t st, const DevFrame& f, const RsQ& q, uint32_t* const bufs[6], F4* key_a, F4* key_b) {
    hipLaunchKernelGGL(k_rs_p3_keys, dim3(q.G), dim3(kBlock), 0, st, f, q, rs_bufs(bufs), RsKeys{key_a, key_b});
}
void launch_rs_p3_select(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, const CameraGPU* cam, uint32_t* const bufs[6], uint32_t* shcnt, F4* key_a, F4* key_b) {
    if (key_a) { hipLaunchKernelGGL(k_rs_p3_select_keys, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cam, rs_bufs(bufs), RsKeys{key_a, key_b}, shcnt); return; }
    hipLaunchKernelGGL(k_rs_p3_select, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, cam, rs_bufs(bufs), shcnt);
}
void launch_rs_p3_merge(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, uint32_t* const bufs[6], uint32_t* shcnt) {
    hipLaunchKernelGGL(k_rs_p3_merge<false>, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, rs_bufs(bufs), shcnt);
    hipLaunchKernelGGL(k_rs_p3_merge<true>, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, rs_bufs(bufs), shcnt);
}
void launch_rs_p3_shade(hipStream_t st, const DevScene& sc, const DevFrame& f, const RsQ& q, uint32_t* const bufs[6], F4* accum) {
    hipLaunchKernelGGL(k_rs_p3_shade, dim3(q.G), dim3(kBlock), 0, st, sc, f, q, rs_bufs(bufs), accum);
}
void launch_accumulate(hipStream_t st, uint32_t max_blocks, const DevFrame& f, const DevPaths& p, F4* accum, const unsigned long long* prim_hits) {
    dispatch_bool(prim_hits != nullptr, [&](auto ph) { hipLaunchKernelGGL((k_accumulate<false, decltype(ph)::value>), dim3(grid_for(f.npl, max_blocks)), dim3(kBlock), 0, st, f, p, accum, AdaptState{}, prim_hits); });
}
void launch_accumulate_list(hipStream_t st, uint32_t max_blocks, const DevFrame& f, const DevPaths& p, F4* accum, const AdaptState& ad, const unsigned long long* prim_hits) {
    dispatch_bool(prim_hits != nullptr, [&](auto ph) { hipLaunchKernelGGL((k_accumulate<true, decltype(ph)::value>), dim3(grid_for(f.npl, max_blocks)), dim3(kBlock), 0, st, f, p, accum, ad, prim_hits); });
}
void launch_adaptive_error(hipStream_t st, const DevFrame& f, const F4* accum, const AdaptState& ad, float threshold, float dark_floor) {
    hipLaunchKernelGGL(k_adaptive_error, dim3(f.chunks_per_sample), dim3(kBlock), 0, st, f, accum, ad, threshold, dark_floor);
}
void launch_adaptive_compact(hipStream_t st, const DevFrame& f, const AdaptState& ad, uint32_t max_spp, uint32_t* list, uint32_t* out5) {
    hipLaunchKernelGGL(k_adaptive_compact, dim3(1), dim3(kCompactBlock), 0, st, f, ad, max_spp, list, out5);
}
// mguides != nullptr: the form that writes the map-guide record too
void launch_denoise_guides(hipStream_t st, uint32_t max_blocks, const DevScene& sc, uint32_t width, uint32_t height, const CameraGPU* cam, F4* guides, F4* mguides) {
    dispatch_bool(sc.tri_cut != nullptr, [&](auto cut) { dispatch_bool(mguides != nullptr, [&](auto maps) {
        hipLaunchKernelGGL((k_denoise_guides<decltype(cut)::value, decltype(maps)::value>), dim3(grid_for(width * height, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, width, height, cam, guides, mguides); }); });
}
uint32_t denoise_workgroups(uint32_t width, uint32_t height) { return ((width + kDnTileW - 1u) / kDnTileW) * ((height + kDnTileH - 1u) / kDnTileH); }
// which form a level runs: go(S, FIRST) with S = the level's step where it is staged (1, 2 or 4 and `staged`), else 0
template <class Go> static void denoise_level_form(const DenoiseLevel& a, bool staged, Go go) {
    if (a.first) { if (staged && a.step == 1u) go(IntC<1>{}, BoolC<true>{}); else go(IntC<0>{}, BoolC<true>{}); }      // (the first level is the only one with step 1)
    else if (staged && a.step == 2u) go(IntC<2>{}, BoolC<false>{});
    else if (staged && a.step == 4u) go(IntC<4>{}, BoolC<false>{});
    else go(IntC<0>{}, BoolC<false>{});
}
// every form of both filters: FL from the two bits of flags (RTX_DENOISE_ALBEDO | RTX_DENOISE_MAPPED_NORMALS), VAR from variance
void launch_denoise_level(hipStream_t st, DenoiseLevel a, bool variance, float sigma_var, uint32_t flags, const F4* in, const F4* half, const F4* guides, const F4* mguides, F4* out, uint32_t* partial, bool staged) {
    a.tiles_x = (a.width + kDnTileW - 1u) / kDnTileW;
    const dim3 grid(denoise_workgroups(a.width, a.height));
    dispatch_bool((flags & kDnAlbedo) != 0u, [&](auto alb) { dispatch_bool((flags & kDnMappedNormals) != 0u, [&](auto nm) { dispatch_bool(variance, [&](auto var) {
        constexpr uint32_t FL = (decltype(alb)::value ? kDnAlbedo : 0u) | (decltype(nm)::value ? kDnMappedNormals : 0u);
        denoise_level_form(a, staged, [&](auto ss, auto first) { hipLaunchKernelGGL((k_denoise_level<decltype(ss)::value, decltype(first)::value, FL, decltype(var)::value>), grid, dim3(kBlock), 0, st, a, sigma_var, in, half, guides, mguides, out, partial); });
    }); }); });
}
void launch_denoise_var_input(hipStream_t st, uint32_t width, uint32_t height, bool albedo, const F4* in, const F4* half, const F4* guides, const F4* mguides, float* out2) {
    DenoiseLevel a{};
    a.width = width; a.height = height; a.step = 1u; a.first = 1u; a.tiles_x = (width + kDnTileW - 1u) / kDnTileW;
    dispatch_bool(albedo, [&](auto alb) { hipLaunchKernelGGL(k_denoise_var_input<decltype(alb)::value>, dim3(denoise_workgroups(width, height)), dim3(kBlock), 0, st, a, in, half, guides, mguides, out2); });
}
void launch_denoise_count(hipStream_t st, const uint32_t* partial, uint32_t n, uint32_t* out) {
    hipLaunchKernelGGL(k_denoise_count, dim3(1), dim3(kBlock), 0, st, partial, n, out);
}
void launch_srgb8(hipStream_t st, const F4* accum, uint32_t npix, uint32_t* out) {
    hipLaunchKernelGGL(k_srgb8, dim3((npix + kBlock - 1) / kBlock), dim3(kBlock), 0, st, accum, npix, out);
}
void launch_debug_layer(hipStream_t st, uint32_t max_blocks, const DevScene& sc, uint32_t width, uint32_t height, const CameraGPU* cam, uint32_t layer, uint32_t* out) {
    // (a scene with a cut-out triangle has tri_uv set: the one CUT form is the TEX one)
    if (sc.tri_cut) { hipLaunchKernelGGL((k_debug_layer<true, true>), dim3(grid_for(width * height, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, width, height, cam, layer, out); return; }
    dispatch_bool(sc.tri_uv != nullptr, [&](auto tex) { hipLaunchKernelGGL(k_debug_layer<decltype(tex)::value>, dim3(grid_for(width * height, max_blocks)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, width, height, cam, layer, out); });
}
void launch_pack_tiles(hipStream_t st, uint32_t max_blocks, const DevFrame& f, const F4* accum, F4* slab) {
    hipLaunchKernelGGL(k_pack_tiles, dim3(grid_for(f.npl, max_blocks)), dim3(kBlock), 0, st, f, accum, slab);
}
void launch_unpack_tiles(hipStream_t st, uint32_t max_blocks, const DevFrame& f, uint32_t nshards, const F4* slabs, F4* accum) {
    hipLaunchKernelGGL(k_unpack_tiles, dim3(grid_for(f.npl * nshards, max_blocks)), dim3(kBlock), 0, st, f, nshards, slabs, accum);
}
void launch_dbg_trace(hipStream_t st, const DevScene& sc, const F4* rays, uint32_t n, int any, F4* hits) {
    dispatch_bool(sc.tri_cut != nullptr && (any == 0 || any == 1), [&](auto cut) { hipLaunchKernelGGL(k_dbg_trace<decltype(cut)::value>, dim3(grid_for(n, 2048)), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, rays, n, any, hits); });
}
void launch_dbg_surface(hipStream_t st, const DevScene& sc, const F4* rays, const F4* hits, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_surface, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, rays, hits, n, out);
}
void launch_dbg_bsdf_eval(hipStream_t st, const DevScene& sc, uint32_t mat, uint32_t flags, const float* in9, uint32_t n, float* out8) {
    hipLaunchKernelGGL(k_dbg_bsdf_eval, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, mat, flags, in9, n, out8);
}
void launch_dbg_bsdf_sample(hipStream_t st, const DevScene& sc, uint32_t mat, uint32_t flags, const float* in8, uint32_t n, float* out8) {
    hipLaunchKernelGGL(k_dbg_bsdf_sample, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, mat, flags, in8, n, out8);
}
void launch_dbg_tex_sample(hipStream_t st, const DevScene& sc, uint32_t tex, const float* uv2, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_tex_sample, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, tex, uv2, n, out);
}
void launch_dbg_albedo(hipStream_t st, const DevScene& sc, const F4* hits, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_albedo, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, hits, n, out);
}
void launch_dbg_opacity(hipStream_t st, const DevScene& sc, const F4* hits, uint32_t n, float* out2) {
    hipLaunchKernelGGL(k_dbg_opacity, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, hits, n, out2);
}
void launch_dbg_shading_normal(hipStream_t st, const DevScene& sc, const F4* rays, const F4* hits, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_shading_normal, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, rays, hits, n, out);
}
void launch_dbg_specular(hipStream_t st, const DevScene& sc, const F4* hits, uint32_t n, float* out8) {
    hipLaunchKernelGGL(k_dbg_specular, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, hits, n, out8);
}
void launch_dbg_ess(hipStream_t st, const DevScene& sc, uint32_t material, const float* pr, const float* ndotv, uint32_t n, float* out) {
    hipLaunchKernelGGL(k_dbg_ess, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, material, pr, ndotv, n, out);
}
void launch_dbg_emission(hipStream_t st, const DevScene& sc, const F4* hits, uint32_t n, float* out8) {
    hipLaunchKernelGGL(k_dbg_emission, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, hits, n, out8);
}
void launch_dbg_light_sample(hipStream_t st, const DevScene& sc, const uint32_t* seeds2, uint32_t n, float* out12) {
    hipLaunchKernelGGL(k_dbg_light_sample, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, seeds2, n, out12);
}
void launch_dbg_env_sample(hipStream_t st, const DevScene& sc, const uint32_t* seeds2, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_env_sample, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, seeds2, n, out);
}
void launch_dbg_env_eval(hipStream_t st, const DevScene& sc, const float* dirs3, uint32_t n, F4* out) {
    hipLaunchKernelGGL(k_dbg_env_eval, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sc, dirs3, n, out);
}
void launch_dbg_tea(hipStream_t st, uint32_t s0, uint32_t s1, uint32_t n, float* out, uint32_t* seed_out) {
    hipLaunchKernelGGL(k_dbg_tea, dim3(1), dim3(64), 0, st, s0, s1, n, out, seed_out);
}
void launch_dbg_primary(hipStream_t st, const DevFrame& f, const CameraGPU* cam, uint32_t sample_id, F4* rays) {
    dispatch_bool(f.lens_radius > 0.0f, [&](auto lens) { hipLaunchKernelGGL(k_dbg_primary<decltype(lens)::value>, dim3((f.width * f.height + kBlock - 1) / kBlock), dim3(kBlock), 0, st, f, cam, sample_id, rays); });
}
void launch_dbg_primary_seeds(hipStream_t st, const DevFrame& f, const CameraGPU* cam, uint32_t sample_id, uint32_t* seeds2) {
    dispatch_bool(f.lens_radius > 0.0f, [&](auto lens) { hipLaunchKernelGGL(k_dbg_primary_seeds<decltype(lens)::value>, dim3((f.width * f.height + kBlock - 1) / kBlock), dim3(kBlock), 0, st, f, cam, sample_id, seeds2); });
}
void launch_focus_distance(hipStream_t st, const DevScene& sc, uint32_t width, uint32_t height, const CameraGPU* cam, uint32_t x, uint32_t y, float* out) {
    dispatch_bool(sc.tri_cut != nullptr, [&](auto cut) { hipLaunchKernelGGL(k_focus_distance<decltype(cut)::value>, dim3(1), dim3(kBlock), trace_lds_bytes(sc), st, sc, sc.small, width, height, cam, x, y, out); });
}

}  // namespace rtx

#ifdef RTX_PROFILE_SECTIONS
// tooling entry point of the PROFILE=1 build only (tools/section_profile.py): read (and optionally clear) the section counters
extern "C" int rtx_debug_traversal(unsigned long long* out8, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out8 && hipMemcpyFromSymbol(out8, HIP_SYMBOL(rtx::g_trv), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
    if (reset) { unsigned long long z[8] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rtx::g_trv), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
extern "C" int rtx_debug_sections(unsigned long long* out36, int reset) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out36 && hipMemcpyFromSymbol(out36, HIP_SYMBOL(rtx::g_sec), sizeof(unsigned long long) * 36) != hipSuccess) return -1;
    if (reset) { unsigned long long z[36] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(rtx::g_sec), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif

#ifdef RTX_WAVE_CLOCK
extern "C" int rtx_debug_wave_times(unsigned long long* out, unsigned nwaves, int reset) {      // nwaves <= 65536 (start, end) pairs
    if (hipDeviceSynchronize() != hipSuccess || nwaves > 65536u) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(rtx::g_wgt), sizeof(unsigned long long) * 2 * nwaves) != hipSuccess) return -1;
    if (reset) { void* d = nullptr; if (hipGetSymbolAddress(&d, HIP_SYMBOL(rtx::g_wgt)) != hipSuccess || hipMemset(d, 0, sizeof(unsigned long long) * 2 * 65536) != hipSuccess) return -1; }
    return 0;
}
#endif

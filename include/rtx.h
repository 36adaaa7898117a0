/*
 * rtx.h — C-ABI of the MI355X wavefront path tracer (librtx_hip.so).
 *
 * This is the drop-in boundary for the path-tracing inner loop of ML200/RoyalTracer-DX.
 * The reference has no FFI; its de-facto boundary is "Renderer (C++) <-> shader resource
 * bindings" (Pathtracer/rdn/Renderer.cpp:953-976, 983-1008, heap built at :1195-1581).
 * Every entry point below replaces one of those bindings / host steps and cites it.
 * Plain pointers and sizes only; no C++/torch types; no exceptions cross this boundary.
 *
 * Conventions
 *   - 4x4 matrices: 16 floats, element (row r, col c) of the column-vector matrix at m[c*4+r].
 *     These are exactly the bytes the reference memcpy's into its constant/structured buffers
 *     (DirectXMath row-vector matrices stored row-major == glm column-major; Renderer.cpp:1722-1768,
 *     2091-2121) and that HLSL consumes as `mul(M, float4(p,1))`.
 *   - Material = 128 B (Pathtracer/src/Components/Vertex.h:14-23), Vertex = 28 B (Vertex.h:25-35),
 *     LightTriangle = 80 B (Renderer.h:113-124).
 *   - Return value 0 = ok, negative = RTX_ERR_*; message via rtx_last_error().
 *     (reference: ThrowIfFailed -> std::exception, DXSampleHelper.h:17-23)
 *   - A context is bound to ONE GPU and is not thread-safe; different contexts may be driven from
 *     different threads/processes (reference: single thread, one in-flight frame, Renderer.cpp:717-735).
 *   - There is NO CPU fallback: rtx_create fails with RTX_ERR_NO_DEVICE when HIP cannot open the device.
 */
#ifndef RTX_H
#define RTX_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RTX_OK               0
#define RTX_ERR_INVALID     -1   /* bad argument / inconsistent scene arrays */
#define RTX_ERR_NO_DEVICE   -2   /* HIP runtime or device not available */
#define RTX_ERR_HIP         -3   /* a HIP call failed (message has the HIP error string) */
#define RTX_ERR_STATE       -4   /* call order violated (e.g. render before commit/camera) */
#define RTX_ERR_OOM         -5

typedef struct rtx_ctx rtx_ctx;   /* one per GPU; opaque */

/* Compile-time shader #defines of the reference (Common_v6.hlsl:1-28) + hard-wired host values
   (Main.cpp:25, Renderer.cpp:1730) become one POD handed to rtx_render. */
typedef struct rtx_params {
    uint32_t width, height;   /* DispatchRays dims == image size (Renderer.cpp:646-654) */
    uint32_t spp;             /* samples per pixel added by this call */
    uint32_t sample_base;     /* first sample id s in the seed formula (RayGen_v6_pass1.hlsl:76-77 uses 1) */
    uint32_t max_bounces;     /* path segments per sample (`bounces`, RayGen.hlsl:68,99) */
    uint32_t nee_samples;     /* light samples per bounce (`nee_samples`, Common_v6.hlsl:8) */
    uint32_t rr_start;        /* Russian roulette when bounce index > rr_start (`rr_threshold`, RayGen.hlsl:69,118) */
    uint32_t frame_seed;      /* stands in for uint(time) (RayGen_v6_pass1.hlsl:76-77; Renderer.cpp:1754-1760) */
    uint32_t flags;           /* RTX_FLAG_* */
    uint32_t tile_size;       /* shard tile edge in pixels: a power of two in [16, 1024] (0 => 64); anything else is RTX_ERR_INVALID everywhere */
    uint32_t shard_rank;      /* this context renders tiles t (row-major tile index) with t % shard_count == shard_rank (RTX_FLAG_BLOCK_TILES: one rectangle of tiles instead) */
    uint32_t shard_count;     /* 0 or 1 => whole image */
} rtx_params;

#define RTX_FLAG_LAMBERT_ONLY 1u  /* strategy 0 only, p_d = 1 (BRDF_v6.hlsl:7-70 bypassed) */
#define RTX_FLAG_JITTER       2u  /* legacy sub-pixel jitter (RayGen.hlsl:84-87); v6 shoots pixel corners (pass1:80-82) */
#define RTX_FLAG_TRANSMISSION 4u  /* EXTENSION: strategy 3 (rough dielectric transmission) for materials with dissolve Kd.w < 1 and Ni != 1; the reference
                                     has the strategy as a stub only (BRDF_v6.hlsl:5,28-29,44-47,85-87).  rtx_render only; ignored with LAMBERT_ONLY
                                     and by the literal pass-1 / ReSTIR modes.  Off: every result is the reference-faithful one */

#define RTX_FLAG_BLOCK_TILES  8u  /* sharding: the tiles of a shard form ONE rectangle (the shard_count ranks as a gx x gy grid of blocks, gx * gy = shard_count chosen
                                     for the smallest block perimeter; of two grids with the same perimeter the one with fewer columns) instead of tile t -> rank t mod shard_count.  Same pixels, same image; what changes is who owns
                                     which tile: round-robin balances a path-traced frame, blocks keep the 20-px halo of a ReSTIR frame small (rtx_render_restir).
                                     Every call that takes rtx_params (render, pack / unpack, slab sizes) follows the flag */

/* kernel classes for rtx_stats */
enum { RTX_K_RAYGEN = 0, RTX_K_TRACE = 1, RTX_K_SHADE = 2, RTX_K_SHADOW = 3, RTX_K_ACCUM = 4, RTX_K_SORT = 5,
       RTX_K_BOUNCE = 6 /* fused trace+shade+shadow kernels: k_bounce_small (tiny scenes), k_bounce_bvh (general path) */,
       RTX_K_ADAPT = 7 /* rtx_render_adaptive: the convergence criterion and the compaction of the active list, once per pass */, RTX_K_COUNT = 8 };

typedef struct rtx_stats {
    uint64_t rays_primary, rays_extension, rays_shadow;  /* BVH queries issued by the last rtx_render */
    uint64_t paths;                                       /* pixel-samples started */
    double   kernel_ms[RTX_K_COUNT];                      /* summed hipEvent time per kernel class (timing option on) */
    uint64_t kernel_launches[RTX_K_COUNT];
    uint64_t kernel_items[RTX_K_COUNT];                   /* work items (rays / paths) processed per class */
    double   render_ms;                                   /* hipEvent time of the whole rtx_render on its stream */
    uint32_t bvh_nodes, triangles, lights, materials;
    uint64_t primary_hits;                                /* camera rays that hit the scene (items of the bounce-0 shading launch) */
    uint32_t bvh_refits, bvh_refs;                        /* commits since the last full BVH build that only refitted boxes; leaf entries of the tree (= triangles unless
                                                             spatial splits, RTX_OPT_BVH_SPLIT, reference some from several leaves) */
    uint64_t restir_stale_history_reads;                  /* rtx_render_restir on shards: temporal-pass reads of last frame's history at a pixel where this context does not hold it
                                                             (outside own rectangle + exchanged halo): must be 0, see rtx_restir_pack_halo */
} rtx_stats;

enum { RTX_OPT_KERNEL_TIMING = 1,    /* 0/1: bracket every launch with hipEvents (rtx_stats.kernel_ms) */
       RTX_OPT_PATHS_PER_BATCH = 2,  /* max pixel-samples in flight (queue capacity), default 128 Mi (~17 GB of path state and queues) */
       RTX_OPT_SORT_MATERIALS = 3,   /* 0/1: material-sorted shading (k_shade sorts its sub-queue chunks by material in LDS; default 0: measured slower) */
       RTX_OPT_LDS_NODES = 4,        /* BVH nodes staged in LDS per workgroup (top of tree) */
       RTX_OPT_SMALL_SCENE = 5,      /* 0/1: brute-force pre-test path for scenes of <= 64 triangles (default 1) */
       RTX_OPT_FUSED_BOUNCE = 6,     /* 0/1: with SMALL_SCENE, fuse trace+shade+shadow into one kernel per bounce (default 1) */
       RTX_OPT_BOUNCE_VARIANT = 7,   /* fused tiny-scene kernel, bounces >= 1: 0 = trace phase pushes HITS into a workgroup-wide LDS ring, shading runs on ring entries (full waves);
                                        1 = trace and shade the same 256 queue entries (the round-1 form);
                                        2 (default) = wave-private form: each wave takes 64-entry chunks from an LDS cursor and keeps its own hit ring and shadow-ray ring,
                                            no workgroup barrier inside a bounce (same bits and ray counts as 0 and 1) */
       RTX_OPT_REFILL_MIN = 8,       /* tuning: idle lanes that trigger a refill in the persistent BVH traversal (default 12) */
       RTX_OPT_STACK_PRIVATE = 9,    /* tuning: traversal stack 0 = LDS column, 1 = private (scratch) memory, (2 is accepted and means 0) */
       RTX_OPT_TRACE_SCHED = 10,     /* tuning: wave schedule of the BVH traversal, 0 = while-while, 1-4 = voted node / triangle steps, 5-7 = voted + speculative (default 6) */
       RTX_OPT_GPU_REFIT = 11,       /* 1 (default): a transform-only rtx_commit_scene refits the resident BVH on the GPU; 0: host refit + upload */
       RTX_OPT_RESTIR_WAVEFRONT = 19,/* 1 (default): rtx_render_v6_pass1 / rtx_render_restir run as wavefront stages (csrc/rtx_restir_wave.hpp: stage kernels of <= 128 VGPRs, every
                                        ray traversed by the persistent kernels of the path tracer); 0: the literal form, one thread per pixel and pass like the reference's raygen
                                        shaders (csrc/rtx_restir.hpp).  Byte-identical buffers and images either way */
       RTX_OPT_OCCLUDER_CACHE = 21,  /* 1: in the persistent any-hit traversal a lane first tests the triangle that occluded its previous ray (neighbouring queue entries are neighbouring
                                        pixels aiming at the same light / sample).  Any-hit is existence, so results are identical — and it is MEASURED SLOWER (same box, alternating:
                                        k_trace_shadow 11.63 -> 12.23 ms on C3, 10.21 -> 10.48 on C5, ReSTIR frames +1 %): the extra triangle step per ray costs more than
                                        the early exits save.  Default 0 */
       RTX_OPT_SHADE_DENSE = 23,     /* general path: 1 = k_shade compacts the HITS of its sub-queue through an LDS ring and shades full waves of them (k_shade_dense), 0 (default) = shades
                                        the queue entries in place (lanes whose ray missed idle).  Results identical.  MEASURED, same box alternating: no gain where it was meant to help
                                        (C5, 14-56 % of a bounce's rays miss: k_shade 8.20 vs 8.22 ms — the lanes are lost inside the NEE / BSDF sections, not at their entry) and
                                        slower where nearly every ray hits (C3: 6.51 -> 7.89 ms: two barriers and a second read of the hit record per 256 entries) */
       RTX_OPT_RESTIR_LANES = 22,    /* 2 (default): the pixels of a ReSTIR frame are processed as two independent halves on two streams (passes 1 + 2, then pass 3), so that the
                                        many short dependent launches of one half fill the launch tails of the other; 1: one chain.  Off while RTX_OPT_KERNEL_TIMING is on.
                                        Results identical */
       RTX_OPT_RESTIR_LANE_MIN = 29, /* pixel lists shorter than this many entries run as ONE chain whatever RTX_OPT_RESTIR_LANES says (default 65 536: below that the second stream has
                                        nothing to hide); tests lower it to exercise the cross-stream ordering on small frames */
       RTX_OPT_RESTIR_CHUNKS = 20,   /* tuning: 256-pixel chunks per workgroup (= private sub-queue) of the ReSTIR stages, default 4 */
       RTX_OPT_OVERLAP_SHADOW = 18,  /* 1 (default): general scenes run the shadow-ray kernel of bounce b on a second (internal) stream beside the closest-hit kernel of
                                        bounce b + 1; everything is joined into the context's stream before rtx_render returns.  Off while RTX_OPT_KERNEL_TIMING is on
                                        (overlapping launches have no per-kernel time).  Results identical */
       RTX_OPT_COMPACT_STATE = 16,   /* 1 (default): the separate trace / shade kernels keep ray, throughput and hit records by QUEUE POSITION in two buffer sets (a bounce
                                        writes its survivors densely at their place in the next queue) instead of by path id in place.  Results identical.
                                        The fused tiny-scene kernels do the same with their 48-B path state (origin, direction, throughput; bounce b reads set b & 1, radiance
                                        stays by path id): bounce 0 and the wave-scheduled form of bounces >= 1 (RTX_OPT_BOUNCE_VARIANT 2) have both layouts.  The block-scheduled
                                        forms (RTX_OPT_BOUNCE_VARIANT 0 / 1) keep the state by path id, in place: a frame rendered with one of them uses that layout throughout,
                                        bounce 0's output included, whatever this option says.  Costs memory: two sets of G x qcap entries, about 3 x the bytes of the in-place
                                        state on a tapered frame.  Measured in profiles/small_compact_time.md */
       RTX_OPT_WORK_STEALING = 15,   /* 1: a wave of the general-scene trace kernels whose sub-queue is exhausted continues with other sub-queues (global chunk cursors + an
                                        exhausted bitmap, pseudo-random victims) instead of draining.  Bit-identical; wave iterations fall 8 % (busy lanes 50.3 -> 55.7 of 64)
                                        but the frame is SLOWER (C3 56.6 vs 47.4 ms, C5 51.0 vs 44.7 ms): the tail iterations it removes are latency-bound and cost few issue
                                        slots next to the other workgroups' full waves, while with stealing every wave of the launch reaches its tail at the same time.
                                        Default 0 */
       RTX_OPT_FUSED_BVH = 14,       /* 1: general (BVH) scenes run trace -> shade -> shadow of all bounces in ONE launch per batch (k_bounce_bvh, phases separated by workgroup
                                        barriers).  Bit-identical, but MEASURED SLOWER than one launch per phase and bounce (C3 51.3 vs 47.7 ms, C5 46.2 vs 44.4 ms: a wave that has
                                        finished its phase keeps its SIMD slot while it waits for the slowest wave of its workgroup, and the kernel needs 86 VGPRs where the
                                        traversal kernels need 75), so the default is 0.  Needs RTX_OPT_TRACE_SCHED 5-7 */
       RTX_OPT_LPT_ORDER = 13,       /* tuning: 1 (default) = the fused tiny-scene kernels take their sub-queues longest first (shorter launch tails), 0 = in index order */
       RTX_OPT_TAPER = 25,           /* 1 (default) = the sub-queues of a batch get shorter towards the end of the dispatch order (weights 8 | 4 | 2 | 1 over the
                                        index ranges G/2 | G/4 | G/8 | G/8), so that the last workgroups of every launch are short ones; 0 = equal sub-queues; 2-8 = that many weight classes.
                                        Never changes a result */
       RTX_OPT_MERGE_RAYS = 24,      /* tuning, general scenes: a launch of the persistent traversal kernels that is predicted (from the previous rtx_render's counters) to hold fewer than
                                        this many rays per sub-queue gives each workgroup 2 / 4 / 8 consecutive sub-queues, down to one round of resident workgroups (the late bounces of
                                        a frame, after Russian roulette).  Default 1024; 0 = one sub-queue per workgroup always.  Never changes a result */
       RTX_OPT_OCTANT_SORT = 32,     /* 1: general scenes, compact state: the closest-hit kernel of bounce b >= 1 fetches the rays of its sub-queue grouped by direction octant (k_shade notes a survivor's
                                        octant, a prologue of the traversal kernel counting-sorts the sub-queue's entries by it).  3: the key is the cell of the ray's ORIGIN on a 256-cell grid over the scene's box, from bounce 2.
                                        2 and 5 are measurement variants (all keys zero; hashed keys).  Never changes a result; MEASURED slower in every form: profiles/r04_octsort_ab.md.  Default 0 */
       RTX_OPT_PARTIAL_REFIT = 37,   /* 1 (default): a transform-only commit re-derives the triangles of the instances whose transform changed and re-quantises only the nodes above them
                                        (the first refit after a build is a full one); 0: every refit touches the whole tree */
       RTX_OPT_LDS_NODES_CLOSEST = 36, /* BVH nodes staged in LDS by the path tracer's CLOSEST-HIT launches; default -1 = auto: for trees of at most 16 MB the first three levels of the wide tree (73 nodes)
                                        while six workgroups per CU remain (the shadow launches keep RTX_OPT_LDS_NODES' choice: more workgroups, fewer nodes); 0 = as the shadow launches.  Takes effect with the next rtx_commit_scene */
       RTX_OPT_RESTIR_KEYS = 35,     /* 1 (default): after passes 1 + 2 every pixel writes what a NEIGHBOUR's test of the spatial pass reads (x1, n1, material, validity flags, M; the GI sample) into
                                        two 32-B records, and the selection stage of pass 3 (up to 18 random neighbours per pixel) reads those instead of the 60-B + 40-B + 40-B records.
                                        Byte-identical; wavefront form only.  0: the selection reads the full records */
       RTX_OPT_NODE_STRIDE = 34,     /* how the traversal finds a BVH node in HBM.  80: the nodes as built, 80 B apart.  128: a copy with one node per 128-B cache line (no node straddles a line), refreshed
                                        after every build / refit.  0 (default) = auto: the copy is made for trees above 16 MB and fetched by the path tracer's closest-hit launches of bounces >= 1
                                        only (street scene, 3.8 M triangles: k_trace_closest -2.4 %; coherent rays and small trees prefer the dense layout: profiles/r04_node_stride_ab.md).
                                        Never changes a result.  Takes effect with the next rtx_commit_scene */
       RTX_OPT_SAMPLE_INTERLEAVE = 33, /* general scenes (k_raygen): which path sits where in the sub-queues.  0: a chunk of 256 queue entries is 256 pixel slots of ONE sample; 1 (default): 256 / S pixel
                                        slots x S consecutive samples with a pixel's samples in neighbouring lanes, S = the largest power of two <= 16 dividing the batch's sample count: the rays
                                        of a wave start closer together at every bounce (C5 k_trace_closest 18.4 -> 17.5 ms, C3 20.6 -> 20.1: profiles/r04_interleave_ab.md).
                                        Never changes a result: seeds come from pixel and sample id, sums are per path */
       RTX_OPT_ASYNC = 31,           /* 1: on a caller-bound stream (rtx_set_stream) rtx_render returns once the frame is ENQUEUED; rtx_pack_tiles / rtx_unpack_tiles (and the caller's collective)
                                        follow it in stream order with no host join in between.  Statistics (rtx_get_stats) and every other entry point join the frame first.  Default 0:
                                        rtx_render returns with the frame finished.  On the context's own stream the option is ignored */
       RTX_OPT_TRACE_COUNTERS = 30,  /* 1: the persistent traversal kernels count node steps and triangle tests (their generic instantiations; a few per cent slower), read with
                                        rtx_debug_trace_counters: work per ray for the bench record.  Default 0.  Never changes a result */
       RTX_OPT_BVH_REINSERT = 26,    /* BVH builder: passes of the insertion-based topology optimisation after the top-down SAH build (Bittner et al. 2013; default see DESIGN.md section 6c).
                                        Changes the tree, never a result; the next rtx_commit_scene rebuilds */
       RTX_OPT_BVH_SPLIT = 27,       /* BVH builder: spatial splits (Stich et al. 2009) where an object split leaves its two sides overlapping by more than value * 1e-9 of the scene's surface
                                        area; 0 (default) = never.  A split triangle is referenced from several leaves; closest hit = minimum over all triangles and any hit = existence,
                                        so no result changes.  The next rtx_commit_scene rebuilds */
       RTX_OPT_ANYHIT_ORDER = 28,    /* any-hit (shadow / visibility) rays visit the hit children of a node in 0 = slot order, 1 = nearest octant first, 2 = farthest octant first;
                                        -1 (default) = what a commit-time probe of 2 048 NEE-like segments on the host found cheapest for this scene and its lights.  Never changes a result */
       RTX_OPT_GPU_BUILD = 38,       /* 1: a geometry-changing rtx_commit_scene builds the BVH ON THE GPU (csrc/rtx_build.hip: Morton sort, PLOC clustering down to <= 16 384 clusters, the top
                                        of the tree by the host's SAH builder + re-insertion over those clusters, SAH collapse to 8-wide nodes and layout on the device, then the refit
                                        kernels) instead of on the host: what the reference's driver does for it in BottomLevelASGenerator.cpp:178-247 / TopLevelASGenerator.cpp:149-250.
                                        0 (default): host build.  Results never depend on the tree; the host-side mirror of the tree (scene cache save, host refit) is not kept */
       RTX_OPT_DEFORM_REBUILD = 40,  /* what a commit after rtx_update_mesh_vertices does to the tree.  0 (default): refit (the boxes follow the vertices, the topology stays); 1: rebuild, through
                                        whichever builder RTX_OPT_GPU_BUILD selects; N >= 2: refit, then rebuild in the same commit if the tree's visit cost (rtx_debug_tree_cost) exceeds
                                        N per cent of its value right after the last build (GPU-refit path only: a tiny scene or RTX_OPT_GPU_REFIT 0 refits on the host, where no cost
                                        is kept).  Never changes a result */
       RTX_OPT_STACK_CAP = 39,       /* 11 (default): traversal-stack entries per lane that live in LDS; a tree whose exact stack bound is deeper keeps the rest in per-lane columns in
                                        global memory, so that LDS (the staged top of the tree, workgroups per CU) is sized for what almost every ray needs.  0 = the whole stack in LDS (until round 5).
                                        Never changes a result.  Takes effect with the next rtx_commit_scene */
       RTX_OPT_SHARED_PRIMARY = 41,  /* 1 (default): fused tiny-scene path without RTX_FLAG_JITTER: all samples of a pixel shoot the same camera ray, so the primary hit and the surface
                                        there are computed once per pixel and rtx_render call (k_primary_surface) instead of once per sample; raygen only enqueues the ids of the hitting paths and
                                        bounce 0 starts from the pixel's record, with sample and seeds derived from the path id.  0: every sample traces and reconstructs its own.  Never changes a result.  rays_primary still counts
                                        one camera ray per sample */
       RTX_OPT_DENOISE_LDS_STEP = 42,/* tuning, rtx_denoise: the levels with step <= this value (0, 1, 2 or 4) stage their tile and its halo in LDS, the coarser ones read every tap from global memory.
                                        Default 4: every step that fits (measured faster than the direct form at steps 1, 2 and 4: profiles/denoise_time.md).  Never changes a result */
       RTX_OPT_SMALL_SLABS = 43,     /* 1 (default): tiny scenes: a pair of pre-test records that are both (near-)parallelograms is tested by two slabs per record, |w . P - c| <= h, instead of four edge
                                        planes (fewer packed instructions per pair; csrc/rtx_small_scene.cpp has the proof that it is as conservative).  0: every pair by its edge planes — the same
                                        kernels, a wave-uniform branch never taken.  Never changes a result; takes effect with the next frame */
       RTX_OPT_BLOCKS_PER_CU = 12    /* tuning: workgroups (= private sub-queues) per compute unit; default 0 = auto: 40 (tiny scenes) / 32 at full frame size (8 measured 4-7 % slower there: tail imbalance), fewer — down to 8 — when a batch is so
                                        small (a shard) that a sub-queue would start with fewer than ~16 / ~8 chunks of 256 paths */ };

/* lifetime: replaces LoadPipeline/device creation (Renderer.cpp:106-254) and OnDestroy (:546-552) */
int  rtx_create(int device_ordinal, rtx_ctx** out);
void rtx_destroy(rtx_ctx*);
const char* rtx_last_error(rtx_ctx*);          /* ctx may be NULL: the CALLING THREAD's last error of a context-free call (rtx_create, rtx_shard_slab_bytes, rtx_restir_state_slab_bytes) */
int  rtx_set_option(rtx_ctx*, int option, int64_t value);
/* run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream.
   replaces the single m_commandQueue (Renderer.cpp:192-199) */
int  rtx_set_stream(rtx_ctx*, void* hip_stream);   /* a caller-owned stream must outlive the work enqueued on it; rtx_destroy does not touch it */

/* t5 `materials` StructuredBuffer<Material>, 128 B stride (Renderer.cpp:373-389, 1287-1296) */
int  rtx_set_materials(rtx_ctx*, const void* mats128, uint32_t count);
/* t2 `BTriVertex` (28 B stride) + t1 `indices` (u32) per model (CreateVB, Renderer.cpp:1973-2072) and the
   model's slice of t4 `materialIDs` (one id per index, Renderer.cpp:391-407).  Vertex.normal.w must equal the
   number of material ids added before this mesh (ObjLoader.h:466 / Hit_v6.hlsl:17). */
int  rtx_add_mesh(rtx_ctx*, const void* verts28, uint32_t nverts, const uint32_t* indices, uint32_t nidx,
                  const uint32_t* material_ids, uint32_t* mesh_out);
/* m_instances.push_back({BLAS, matrix}) (Renderer.cpp:908-921); instance id = order of insertion (:843-845) */
int  rtx_add_instance(rtx_ctx*, uint32_t mesh, const float o2w[16], uint32_t* inst_out);
/* t3 `instanceProps` update (UpdateInstancePropertiesBuffer, Renderer.cpp:2091-2121; prevObjectToWorld := the old matrix);
   needs rtx_commit_scene again, which then only REFITS the BVH boxes (TLAS refit, Renderer.cpp:594) instead of rebuilding */
int  rtx_set_instance_transform(rtx_ctx*, uint32_t inst, const float o2w[16]);
/* instanceDescs[i].InstanceMask (TopLevelASGenerator.cpp:198; every TraceRay of the reference passes 0xFF): visible = 0 is mask 0 — the instance exists for no ray, closest
   hit or any hit, its emissive triangles are no lights (rtx_get_lights, rtx_stats.lights), and every result is bit-identical to the scene without it — while instance ids and
   global triangle ids stay what they were (hits4, debug layer 14, SampleData.objID, the instance word of a light record; rtx_stats.triangles stays the total).  All or
   nothing: no per-ray-type masks.  Every instance starts visible; valid before the first commit and on a resident scene.  Like rtx_set_instance_transform it needs
   rtx_commit_scene again (rendering in between is RTX_ERR_STATE), and on a resident scene that commit is never a rebuild: a REFIT (rtx_stats.bvh_refits + 1) that re-derives
   the instance's triangles as never-hit records and takes them out of (or puts them back into) the boxes above them, so rays neither hit hidden triangles nor pay for them; it
   may share the commit with transform changes and vertex updates, of the same instance too.  The tree's topology is always the one built over ALL instances, and hide -> commit
   -> show -> commit restores the device tree to the bit (rtx_debug_tree_hash).  An unknown instance is RTX_ERR_INVALID and leaves the scene committed and untouched; the
   value the instance already has is accepted and dirties nothing.  A geometry-changing commit (rtx_add_instance, builder options, RTX_OPT_DEFORM_REBUILD 1) keeps every
   instance's visibility.  SPAWN POOL: add the objects a scene will ever need up front, hidden, and commit once; showing one later costs a partial refit plus, if it carries
   emitters, the light scan, where rtx_add_instance costs a rebuild.
   Paths: the host builder's tree (also RTX_OPT_GPU_REFIT 0, the host refit) gets one full pass of the GPU refit kernels behind its upload while anything is hidden, so hidden
   triangles are culled from the boxes there too; a tiny scene (<= 64 triangles) with a hidden instance runs on the general BVH path until everything is visible again (its
   pre-test records are derived from geometry; results are identical by the parity contract).  The ReSTIR history is left alone, as after a vertex update: call
   rtx_restir_reset for a frame without ghosting.  rtx_save_scene_cache with any hidden instance is RTX_ERR_STATE (the file holds no visibility); a loaded cache has everything
   visible. */
int  rtx_set_instance_visible(rtx_ctx*, uint32_t inst, int visible);
/* New vertex data for a mesh whose topology stays: nverts must equal the mesh's, indices and material ids are kept, Vertex.normal.w must be
   what it was (the mesh's materialIDs base).  Positions AND normals are taken.  Needs rtx_commit_scene again, which then re-derives only the
   triangles of this mesh's instances and refits (BottomLevelASGenerator.cpp:185-209, updateOnly) instead of rebuilding (RTX_OPT_DEFORM_REBUILD).
   RTX_ERR_INVALID (unknown mesh, other vertex count, changed normal.w, null pointer) leaves the scene untouched and committed.  The ReSTIR history is
   left alone (the temporal pass reprojects through prevObjectToWorld only): call rtx_restir_reset for a frame without ghosting. */
int  rtx_update_mesh_vertices(rtx_ctx*, uint32_t mesh, const void* verts28, uint32_t nverts);
/* DIFFUSE TEXTURE MAPS (new; the reference parses map_Kd and samples nothing: an extension, unpinned by definition like strategy 3 and pinned by its own properties
   in tests/test_texture.py).  rtx_render and rtx_render_adaptive only; rtx_render_v6_pass1 and rtx_render_restir ignore maps, as they ignore RTX_FLAG_TRANSMISSION.
   DATA.  Per mesh an optional array of one (u, v) float pair per INDEX entry, parallel to `indices` and `material_ids`: per corner, not per vertex (the 28-byte Vertex
   stays as it is); a mesh without the array has (0, 0) at every corner.  Per context a table of textures, each width x height RGBA8 (r in the first byte), row 0 on
   top, alpha read by the opacity slot only (ALPHA CUT-OUTS below), 1 <= width, height <= 16384 (and at most 2^31 texels in the whole table); RTX_TEX_SRGB says the bytes are sRGB-encoded.  Per material the
   slot RTX_MAP_KD: a texture id or -1.
   BYTE -> FLOAT.  A 256-entry float32 table per encoding, filled on the host.  Linear: T[b] = (float)b / 255.0f.  sRGB, in double: c = b / 255.0;
   c <= 0.04045 ? c / 12.92 : pow((c + 0.055) / 1.055, 2.4); rounded to float32 once.
   Sample(tex, s, t), float32 in exactly this order, no contraction, W x H the texture's size:
       fs = s - floorf(s);  ft = t - floorf(t)                                            (repeat wrap)
       x  = fs * (float)W - 0.5f;  y = (1.0f - ft) * (float)H - 0.5f                      (OBJ's v runs upward)
       x0 = floorf(x);  y0 = floorf(y);  fx = x - x0;  fy = y - y0
       ix0 = wrap((int)x0, W);  ix1 = wrap((int)x0 + 1, W);  iy0, iy1 likewise;  wrap(i, n) = ((i % n) + n) % n
       per channel k = r, g, b, with cab = T[texel(ixa, iyb).k]:
       top = c00 + fx * (c10 - c00);  bot = c01 + fx * (c11 - c01);  c = top + fy * (bot - top)
   There are NO MIP LEVELS: a path tracer integrates the pixel footprint by sampling, and every sample reads the full-resolution image.
   PER HIT on a surface whose material m has RTX_MAP_KD = tex >= 0, with (u, v) the hit record's barycentrics and uv0, uv1, uv2 the triangle's corner pairs:
       b0 = 1.0f - u - v
       s  = (b0 * uv0.x + u * uv1.x) + v * uv2.x ;  t likewise with .y
       tl = Sample(tex, s, t)
       Kd'[k]   = half_round(m.Kd[k] * tl[k])                                             (binary16 round trip, the MaterialOptimized rounding of the table's Kd)
       KdPi'[k] = Kd'[k] / PI                                                             (IEEE division, as for the table)
   KdPi' replaces the material's Kd / PI wherever the shading reads the diffuse colour at that hit: the Lambert term of the mixture BSDF, for the NEE samples and for the
   continuation.  Everything else stays the material's: Ks, Ke, Pr, Pm, dissolve, the light list, the strategy probabilities, the random-number sequence (unless SPECULAR MAPS, below).  An emissive
   material's map_Kd has no effect (emitters are not shaded; its emission is textured by EMISSION MAPS, below).  CONSEQUENCE: a scene in which every textured triangle sees one value tl is, bit for bit, the untextured scene
   whose triangles carry materials with Kd = Kd'.  rtx_denoise is unchanged (its colour edge-stop now sees texture detail, unless RTX_DENOISE_ALBEDO demodulates by Kd': DENOISING, MAP GUIDES); debug layer 13 shows Kd'.
   CALLS.  rtx_set_mesh_uvs: nidx pairs, nidx = the mesh's index count; NULL clears.  rtx_set_texture: tex <= the current count, == count appends; the texels are copied.
   rtx_set_material_map: slot RTX_MAP_KD (or RTX_MAP_OPACITY, below), tex -1 = none.  RTX_ERR_INVALID — unknown mesh, material, texture or slot; nidx other than the mesh's; a non-finite UV; a size
   outside the limits; unknown flag bits; a NULL pixel pointer — leaves the scene untouched and committed.  rtx_set_materials resets every map to -1 (the table is
   replaced).  Like rtx_set_instance_visible the three are valid before the first commit and on a resident scene, and need rtx_commit_scene again (rendering in between is
   RTX_ERR_STATE).  On a resident general scene a commit after these calls alone uploads tables only: no rebuild, no refit, rtx_stats.bvh_refits and rtx_debug_tree_hash
   unchanged; it may share a commit with transform, visibility and vertex edits.  rtx_update_mesh_vertices keeps a mesh's UVs; geometry-changing commits and
   RTX_OPT_GPU_BUILD keep everything (global triangle ids do not depend on the tree).  rtx_save_scene_cache while any material has a map is RTX_ERR_STATE (the file holds
   no texels); a loaded cache has no maps and no textures.  A tiny scene (<= 64 triangles) runs on the general BVH path while a material that a triangle uses has a map;
   the commit that crosses that line, either way, is a rebuild.  With such a map active rtx_render runs the default separate kernels whatever RTX_OPT_FUSED_BVH,
   RTX_OPT_SHADE_DENSE and RTX_OPT_SORT_MATERIALS say (measured-and-rejected variants get no textured copy); RTX_OPT_COMPACT_STATE 0 and 1 both work. */
/* ALPHA CUT-OUTS (new; the reference parses map_d and samples nothing: an extension like map_Kd, pinned by its own definition and properties in tests/test_cutout_ref.py /
   tests/test_cutout.py).  Foliage, chains, fences and decals are quads whose shape lives in the alpha channel of a texture: whether a ray HIT depends on a texel, so the
   test runs inside the traversal.
   SLOT.  rtx_set_material_map(ctx, material, RTX_MAP_OPACITY, tex) binds a texture of the table above (RTX_MAP_OPACITY = 2; the value 1 was an unknown slot before this
   slot existed and stays one, so that no call that was refused is accepted now).  The opacity slot reads that texture's ALPHA BYTE (the 4th byte of a
   texel); one RGBA8 texture may serve both slots of a material.
   CUT-OUT TRIANGLE.  A triangle whose material (the id of its first index entry) has RTX_MAP_OPACITY >= 0 and no component of Ke > 0.  An emitter's opacity map has no effect,
   as its map_Kd has none: the light list, its CDF and rtx_get_lights are untouched.
   ALPHA AT A GEOMETRIC HIT with barycentrics (u, v) on global triangle prim, uv0..2 its corner pairs; float32 in exactly this order, no contraction:
       b0, s, t exactly as in PER HIT above;  x0, y0, fx, fy, ixa, iyb exactly as in Sample(tex, s, t) (repeat wrap, v upward, wrap())
       a_ab = T_linear[alpha byte of texel(ixa, iyb)]                                     (the LINEAR table (float)b / 255.0f, whatever RTX_TEX_SRGB says)
       top = a00 + fx * (a10 - a00);  bot = a01 + fx * (a11 - a01);  a = top + fy * (bot - top)
   The hit is ACCEPTED iff a >= 0.5f.  The cut-off is fixed: there is no per-material cut-off, and no fractional (stochastic) opacity.
   HIT RULE.  A candidate counts for a ray iff the triangle test passes (determinant floor, exclusive (tmin, tmax)) AND the triangle is not a cut-out triangle or its alpha
   is accepted.  Closest hit stays "minimum t, ties to the lower global triangle id", now over accepted candidates only; any hit is the existence of an accepted candidate.
   CONSEQUENCE: a scene in which every cut-out triangle sees alpha on one side of 0.5 over its whole area is, bit for bit, the scene in which the rejected triangles do not
   exist — image, ray counts and hit records, ids keeping their meaning.
   WHO SEES CUT-OUTS.  rtx_render, rtx_render_adaptive, the guides of rtx_denoise, debug layers 10-17, rtx_debug_trace_closest / rtx_debug_trace_any, and rtx_debug_surface /
   rtx_debug_albedo through the hits they are given.  IGNORED BY rtx_render_v6_pass1, rtx_render_restir (their visibility rays included), rtx_debug_trace_stats, the
   commit-time any-hit order probe and the meaning of RTX_OPT_TRACE_COUNTERS' tallies (geometric tests) — as they ignore map_Kd, the environment and RTX_FLAG_TRANSMISSION.
   A hidden instance stays hidden (its geometric test fails first); dissolve and transmission are unrelated and unchanged.
   CALLS AND COMMITS follow the map_Kd rules word for word: valid before the first commit and on a resident scene; rtx_commit_scene again (rendering in between is
   RTX_ERR_STATE); RTX_ERR_INVALID (unknown slot, material or texture) leaves the scene committed and untouched; rtx_set_materials resets the opacity maps to -1; on a resident
   general scene a commit after map calls alone uploads tables only (no rebuild, no refit, rtx_stats.bvh_refits and rtx_debug_tree_hash unchanged: the per-triangle opacity
   table lives beside the leaf records, not in them); vertex updates, transform / visibility edits, geometry-changing commits and RTX_OPT_GPU_BUILD keep cut-outs on their
   triangles; a tiny scene (<= 64 triangles) runs on the general BVH path while any triangle is a cut-out triangle, and the commit that crosses that line is a rebuild;
   rtx_save_scene_cache with an opacity map bound is RTX_ERR_STATE.
   OPTIONS while a cut-out is active: RTX_OPT_FUSED_BVH, RTX_OPT_SHADE_DENSE, RTX_OPT_SORT_MATERIALS, RTX_OPT_WORK_STEALING and RTX_OPT_OCCLUDER_CACHE are ignored (the default
   form runs); RTX_OPT_COMPACT_STATE 0 / 1, RTX_OPT_STACK_PRIVATE, RTX_OPT_STACK_CAP and RTX_OPT_TRACE_SCHED 0-7 all work. */
/* NORMAL MAPS (new; the reference parses norm / map_Bump and samples nothing: an extension like map_Kd, unpinned by the reference, pinned by its own definition and properties in
   tests/test_normalmap_ref.py / tests/test_normalmap.py).  A tangent-space normal map perturbs the SHADING normal of a hit, so that a wall shades less flat than its triangles.
   All device arithmetic is float32 in exactly the written order, no contraction, plain * + - / and sqrtf.
   SLOT.  rtx_set_material_map(ctx, material, RTX_MAP_NORMAL, tex) binds a texture of the table above (RTX_MAP_NORMAL = 4; the values 1 and 3 stay unknown slots).  The RGB
   bytes are a tangent-space normal, OpenGL convention: green = +bitangent = the direction of increasing v.  RTX_TEX_SRGB is ignored for this slot, as the opacity slot ignores it.
   DECODE TABLE.  Nt[b] = max(((float)b - 128.0f) / 127.0f, -1.0f), 256 floats filled on the host: byte 128 is exactly 0, byte 255 exactly 1.
   TANGENT TABLE.  6 floats per GLOBAL triangle id, built on the host at rtx_commit_scene in double from the float32 inputs, each value rounded to float32 once: with p0..2 the
   mesh's current OBJECT-space vertex positions and uv0..2 the triangle's corner pairs (zeros for a mesh without UVs)
       e1 = p1 - p0;  e2 = p2 - p0;  du1 = uv1.x - uv0.x;  dv1 = uv1.y - uv0.y;  du2 = uv2.x - uv0.x;  dv2 = uv2.y - uv0.y;  det = du1 * dv2 - du2 * dv1
       T.k = (e1.k * dv2 - e2.k * dv1) / det;  B.k = (e2.k * du1 - e1.k * du2) / det
   det == 0, or any of the six values not finite after rounding: six zeros.  Object space: a transform-only commit does not touch the table, a commit after
   rtx_update_mesh_vertices re-derives it.  The table exists only while a normal map is active.
   NORMAL-MAPPED HIT.  The hit's material m is not an emitter (an emitter's map has no effect, as for map_Kd) and has RTX_MAP_NORMAL = tex >= 0.  n = the world shading normal of
   the surface reconstruction, M = the instance's objectToWorld (M[4 * column + row]), wo = the ray's direction negated, (u, v) = the hit record's barycentrics:
       b0, s, t exactly as PER HIT of map_Kd;  x0, y0, fx, fy, ixa, iyb exactly as Sample()
       c.k (k = x, y, z from bytes r, g, b): cab = Nt[byte k of texel(ixa, iyb)];  top = c00 + fx * (c10 - c00);  bot = c01 + fx * (c11 - c01);  c.k = top + fy * (bot - top)
       if c.x == 0 and c.y == 0: n' = n                                                  (a flat texel changes NOTHING, to the bit)
       Tw.k = (M[0 + k] * T.x + M[4 + k] * T.y) + M[8 + k] * T.z;  Bw likewise
       dT = (n.x * Tw.x + n.y * Tw.y) + n.z * Tw.z;  tv.k = Tw.k - n.k * dT;  l2 = (tv.x * tv.x + tv.y * tv.y) + tv.z * tv.z
       if not (l2 > 0) or l2 is inf: n' = n
       inv = 1.0f / sqrtf(l2);  t.k = tv.k * inv
       bv = (n.y * t.z - n.z * t.y, n.z * t.x - n.x * t.z, n.x * t.y - n.y * t.x)
       sg = ((bv.x * Bw.x + bv.y * Bw.y) + bv.z * Bw.z) < 0 ? -1.0f : 1.0f               (handedness from the geometry: mirrored UVs and mirrored instances alike)
       m.k = (t.k * c.x + (bv.k * sg) * c.y) + n.k * c.z;  m2 = (m.x * m.x + m.y * m.y) + m.z * m.z
       if not (m2 > 0) or m2 is inf: n' = n;  else n'.k = m.k * (1.0f / sqrtf(m2))
       a = (n.x * wo.x + n.y * wo.y) + n.z * wo.z;  a' likewise with n'
       if (a > 0 and not a' > 0) or (a < 0 and not a' < 0): n' = n                      (the map never turns the surface away from the viewer)
   n' replaces the shading normal for everything the shading does at that hit: the transmission flip, the mixture's view terms, triangle-light and environment NEE, the
   continuation.  Position, flat normal, area, the emissive hit, the light list and the random-number sequence are untouched.  CONSEQUENCE: a scene whose normal maps hold only
   texels with r = g = 128 is, bit for bit, the scene with no normal map bound.
   WHO SEES IT.  rtx_render, rtx_render_adaptive, rtx_debug_shading_normal.  IGNORED BY rtx_render_v6_pass1, rtx_render_restir, the guides of rtx_denoise (its opt-in
   map guides see it: RTX_DENOISE_MAPPED_NORMALS), rtx_read_layer 10-17, rtx_debug_surface and rtx_focus_distance_at — as they ignore map_Kd.
   CALLS AND COMMITS follow the map_Kd rules word for word: valid before the first commit and on a resident scene; rtx_commit_scene again (rendering in between is
   RTX_ERR_STATE); RTX_ERR_INVALID leaves the scene committed and untouched; rtx_set_materials resets the slot to -1; on a resident general scene a map-only commit uploads
   tables only (rtx_stats.bvh_refits and rtx_debug_tree_hash unchanged); a tiny scene (<= 64 triangles) runs on the general BVH path while a non-emitting material that a
   triangle uses has a normal map, and the commit that crosses that line is a rebuild; rtx_save_scene_cache with one bound is RTX_ERR_STATE.  RTX_OPT_FUSED_BVH,
   RTX_OPT_SHADE_DENSE and RTX_OPT_SORT_MATERIALS are ignored while one is active; RTX_OPT_COMPACT_STATE 0 and 1 both work. */
/* SPECULAR MAPS (new; the reference parses map_Ks / map_Pr / map_Pm and samples nothing: an extension like map_Kd, unpinned by the reference, pinned by its own definition and
   properties in tests/test_specmap_ref.py / tests/test_specmap.py).  Three more material-map slots let a texture vary the specular colour, the roughness and the metalness of
   a material over its surface: puddles on a floor, worn metal, glossy mortar.  All device arithmetic is float32 in exactly the written order, no contraction.
   SLOTS.  rtx_set_material_map(ctx, material, RTX_MAP_KS | RTX_MAP_PR | RTX_MAP_PM, tex) binds a texture of the table above (6, 8 and 10; the values 1, 3, 5, 7 and 9 stay
   unknown slots).  Green is roughness and blue is metalness: one packed occlusion-roughness-metal texture serves both slots, and a grey image (r = g = b) serves either.
   PER HIT on a non-emitting material m (an emitter's maps have no effect, as for map_Kd), with b0, s, t exactly as PER HIT of map_Kd and the taps and fx, fy exactly as Sample():
       RTX_MAP_KS = tex >= 0:  tl = Sample(tex, s, t)  (the RGB bytes, RTX_TEX_SRGB honoured as for the Kd slot);   Ks'[k] = half_round(m.Ks[k] * tl[k])
       RTX_MAP_PR = tex >= 0:  g_ab = T_linear[green byte of texel(ixa, iyb)]  (the LINEAR table, whatever RTX_TEX_SRGB says);
                               top = g00 + fx * (g10 - g00);  bot = g01 + fx * (g11 - g01);  g = top + fy * (bot - top);   Pr' = half_round(m.Pr * g)
       RTX_MAP_PM = tex >= 0:  b likewise with the blue byte;   Pm' = half_round(m.Pm * b)
   A slot without a map keeps the table's value.  Ks', Pr', Pm' replace m.Ks, m.Pr, m.Pm wherever the shading reads them at that hit: strategy_probs, the Pr < 0.04 test of
   select_strategy, mix_view (alpha, G1), ggx_eval / ggx_pdf, sample_ggx, and btdf_eval under RTX_FLAG_TRANSMISSION — for the triangle-light NEE, the environment NEE and the
   continuation alike.  Untouched: Kd / Kd', Ke, dissolve, Ni, the light list, the hit, the random-number sequence.  Under RTX_FLAG_LAMBERT_ONLY none of the three is read: the
   frame is the unmapped frame to the bit, and the Lambert kernels that frame launches are launched.
   ENERGY TABLE.  A material's multiscatter look-up (LUT, 16 floats) is generated from ITS roughness; rtx_set_ess_table(ctx, table, rows) hands the library the look-ups of `rows`
   roughnesses so that the energy compensation can follow Pr': row r (16 floats) is the LUT of roughness r / (rows - 1).  2 <= rows <= 256, every value finite; NULL / 0 clears
   the table; RTX_ERR_INVALID leaves everything untouched.  A table edit like the map calls: it needs rtx_commit_scene, a commit after it alone uploads tables only, and
   rtx_set_materials does not clear it.  At a hit whose material has RTX_MAP_PR >= 0, while a table A is set, mix_view takes Ess from the table instead of m.LUT — rows first, so
   that a constant map equals a material:
       fr = Pr' * (float)(rows - 1);  r0 = clamp((int)floorf(fr), 0, rows - 1);  r1 = min(r0 + 1, rows - 1);  wr = fr - (float)r0
       i0, i1, w from NdotV exactly as ess_lut (NdotV saturated, f = NdotV * 15.0f, i0 = (int)floorf(f), i1 = min(i0 + 1, 15), w = f - (float)i0)
       L[i] = A[r0][i] + wr * (A[r1][i] - A[r0][i])     for i = i0, i1
       Ess  = L[i0] + w * (L[i1] - L[i0])
   With no table set, or on a material without a roughness map, m.LUT is read as before: that is then the energy compensation of the TABLE's roughness m.Pr, not of Pr'.
   CONSEQUENCES.  (a) A scene in which every mapped triangle sees one texel value over its whole area is, bit for bit, the unmapped scene whose triangles carry materials with
   Ks', Pr', Pm' — and, where a table is set and the roughness is mapped, with LUT[i] = A[r0][i] + wr * (A[r1][i] - A[r0][i]) for all 16 i.  (b) An all-255 linear map with no
   table set changes nothing, to the bit: the table's values are binary16-rounded already.
   WHO SEES IT.  rtx_render, rtx_render_adaptive, rtx_debug_specular, rtx_debug_ess.  IGNORED BY rtx_render_v6_pass1, rtx_render_restir, rtx_denoise and its map guides,
   rtx_read_layer and the other debug probes — as they ignore map_Kd.
   CALLS AND COMMITS follow the map_Kd / NORMAL MAPS rules word for word: valid before the first commit and on a resident scene; rtx_commit_scene again (rendering in between is
   RTX_ERR_STATE); RTX_ERR_INVALID leaves the scene committed and untouched; rtx_set_materials resets the three slots to -1; on a resident general scene a map-only commit
   uploads tables only (rtx_stats.bvh_refits and rtx_debug_tree_hash unchanged); a tiny scene (<= 64 triangles) runs on the general BVH path while a non-emitting material that
   a triangle uses has one of the three maps, and the commit that crosses that line is a rebuild; rtx_save_scene_cache with one bound is RTX_ERR_STATE.  RTX_OPT_FUSED_BVH,
   RTX_OPT_SHADE_DENSE and RTX_OPT_SORT_MATERIALS are ignored while one is active; RTX_OPT_COMPACT_STATE 0 and 1 both work. */
/* EMISSION MAPS (new; the reference parses map_Ke and samples nothing: an extension like map_Kd, unpinned by the reference, pinned by its own definition and properties in
   tests/test_emimap_ref.py / tests/test_emimap.py).  One more material-map slot lets a texture vary a material's emission over its surface: lanterns, shop signs, screens, lit
   windows — an emissive material whose Ke is white and whose map is mostly black.  All device arithmetic is float32 in exactly the written order, no contraction.
   SLOT.  rtx_set_material_map(ctx, material, RTX_MAP_KE, tex) binds a texture of the table above (12; the value 11 stays an unknown slot, like 1, 3, 5, 7 and 9).  The slot
   reads the RGB bytes and honours RTX_TEX_SRGB, as the Kd slot does.  The map MULTIPLIES the material's Ke.
   EMITTER.  What it always was: a material whose rounded Ke has length > 0.  The map never makes an emitter out of a non-emitter and never a non-emitter out of an emitter: a
   hit on a black texel of an emissive material still ends the path there and adds nothing (emitters are not shaded).  On a non-emitting material the slot has no effect at all.
   AT AN EMISSIVE HIT on global triangle prim, hit barycentrics (u, v), material m with RTX_MAP_KE = tex >= 0: b0, s, t exactly as PER HIT of map_Kd;
       tl = Sample(tex, s, t);   Ke'[k] = half_round(m.KeFull[k] * tl[k])      (the binary16 round trip that the table's Ke is a copy of)
   Ke' replaces Ke in the radiance the hit adds, at bounce 0 and at bounces >= 1, and the MIS weight there replaces (Ke.x + Ke.y + Ke.z) / 3 by the per-triangle q[prim] of the
   table below: pdf_light = (q[prim] / total_weight) * dist2 / max(cos_t, EPS).
   AT A TRIANGLE-LIGHT NEE SAMPLE.  The light record carries its global triangle id and the emission texture of its material.  With u, v, w the sample's weights of corners 0,
   1, 2:  s = (u * uv0.x + v * uv1.x) + w * uv2.x, t likewise;  tl = Sample(tex, s, t);  the contribution uses em[k] * tl[k] where it used em[k] (em = the material's Ke, as
   rtx_get_lights hands it out).  Selection, the three draws, pdf_l, the rejection tests and the shadow ray are unchanged in form; a zero contribution asks for no shadow ray.
   PER-TRIANGLE MEAN AND THE LIGHT WEIGHTS.  Built on the host at rtx_commit_scene, only while an emission map is active (an emitting material that some triangle uses has the
   map).  For each emitter triangle whose material has the map, with W x H the texture's size and uv0..2 the corner pairs:
       n = clamp(ceil(max over the three edges of max(|du| * W, |dv| * H)), 1, 16)      (in double)
   the triangle is cut into n^2 equal sub-triangles; "upright" ones have their centroids at hit barycentrics ((i + 1/3) / n, (j + 1/3) / n) for i + j <= n - 1, "inverted" ones
   at ((i + 2/3) / n, (j + 2/3) / n) for i + j <= n - 2; the order is i outer, j inner, the upright one of a cell before its inverted one.  The centroid barycentrics are rounded
   to float32, then b0, s, t and Sample() run in float32 exactly as on the device.
       mean[k] = (sum of the samples, in double, in that order) / n^2, rounded to float32 once;   E[k] = m.KeFull[k] * mean[k]      (float32)
       weight  = area * ((E.x + E.y + E.z) / 3)      where the light scan has area * inten;   q[prim] = (Eh.x + Eh.y + Eh.z) / 3,  Eh[k] = half_round(E[k])
   Unmapped emitter triangles keep inten and get q[prim] = (Ke.x + Ke.y + Ke.z) / 3 of the rounded copy, so the hit reads one table whatever the material; non-emitting
   triangles and hidden instances get 0.  The rest of the list is built as before from the new weights: sorted descending, ties by collection order, the running CDF ends in
   1.0f; wn, total and pdf_l as before.  WHICH triangles are in the list does not change (rtx_stats.lights and rtx_get_lights' count stay; the 80-byte record keeps its layout
   and its em = the material's Ke): only weights and order do.  A scene whose total weight is 0 (every map black) has no light list for the renderer: no NEE slots, the
   random-number sequence of a scene without lights (rtx_get_lights then reports wn = 0).  The table depends on no transform: a transform-only commit leaves it alone.
   CONSEQUENCES.  (a) A scene in which every mapped emitter triangle sees one texel value c over its whole area, every component of c > 0, is, bit for bit, the unmapped scene
   whose triangles carry materials with Ke = KeFull * c (the mean of n^2 equal floats in double is that float).  (b) An all-255 linear map changes nothing, to the bit.  (c)
   Unbiased whatever the quadrature misses: a triangle with q = 0 that still has a lit texel is found by BSDF sampling with mi = 1.
   WHO SEES IT.  rtx_render, rtx_render_adaptive, rtx_debug_emission, rtx_debug_light_sample.  IGNORED BY rtx_render_v6_pass1, rtx_render_restir, rtx_denoise (emitters pass
   through as ever), rtx_read_layer (layer 16 shows the table's Ke) and the other debug probes — as they ignore map_Kd.
   CALLS AND COMMITS follow the map_Kd rules word for word: valid before the first commit and on a resident scene; rtx_commit_scene again (rendering in between is
   RTX_ERR_STATE); RTX_ERR_INVALID leaves the scene committed and untouched; rtx_set_materials resets the slot to -1; rtx_save_scene_cache with one bound is RTX_ERR_STATE;
   RTX_OPT_FUSED_BVH, RTX_OPT_SHADE_DENSE and RTX_OPT_SORT_MATERIALS are ignored while one is active; RTX_OPT_COMPACT_STATE 0 and 1 both work.  ONE ADDITION: while an emission
   map is active on an emitter, or was at the previous commit, a map-only commit (a map call, rtx_set_texture, rtx_set_mesh_uvs) also rebuilds the light list — still no
   rebuild or refit of the tree (rtx_stats.bvh_refits and rtx_debug_tree_hash unchanged).  A tiny scene (<= 64 triangles) runs on the general BVH path while an emitter that a
   triangle uses has the map, and the commit that crosses that line is a rebuild. */
#define RTX_TEX_SRGB 1u
enum { RTX_MAP_KD = 0, RTX_MAP_OPACITY = 2 };      /* 1 is not a slot: it stays RTX_ERR_INVALID, as it always was */
enum { RTX_MAP_NORMAL = 4 };                       /* ... and neither is 3 */
enum { RTX_MAP_KS = 6, RTX_MAP_PR = 8, RTX_MAP_PM = 10 };      /* ... nor 5, 7, 9 (SPECULAR MAPS) */
enum { RTX_MAP_KE = 12 };                          /* ... nor 11 (EMISSION MAPS) */
int  rtx_set_mesh_uvs(rtx_ctx*, uint32_t mesh, const float* uv2 /* nidx pairs; NULL clears */, uint32_t nidx);
int  rtx_set_texture(rtx_ctx*, uint32_t tex /* <= current count; == count appends */, const void* rgba8, uint32_t width, uint32_t height, uint32_t flags);
int  rtx_set_material_map(rtx_ctx*, uint32_t material, uint32_t slot, int32_t tex /* -1 = none */);
int  rtx_set_ess_table(rtx_ctx*, const float* table /* rows x 16 */, uint32_t rows);      /* SPECULAR MAPS, ENERGY TABLE; NULL / 0 clears */
/* tests: SPECULAR MAPS by the device function k_shade runs — hits4 as rtx_debug_trace_closest writes them -> 8 words per record: Ks'.xyz, Pr', Pm', then the ks / pr / pm
   texture id as uint bits or 0xFFFFFFFF (no map in that slot; an emitter and every hit while no specular map is active: the table's values and three 0xFFFFFFFF); a miss gives
   five zeros and three 0xFFFFFFFF.  rtx_debug_ess: the Ess mix_view would use for `material` at n (Pr', NdotV) pairs — the table path or m.LUT, by the rule above */
int  rtx_debug_specular(rtx_ctx*, const float* hits4, uint32_t n, float* out8);
int  rtx_debug_ess(rtx_ctx*, uint32_t material, const float* pr, const float* ndotv, uint32_t n, float* out);
/* tests: EMISSION MAPS by the device functions k_shade runs.  rtx_debug_emission: hits4 as rtx_debug_trace_closest writes them -> 8 words per record: Ke'.xyz, q[prim], the
   emission texture id as uint bits or 0xFFFFFFFF, 0, 0, 0; a non-emitter or a miss gives zeros and 0xFFFFFFFF (while no emission map is active an emitter gives the table's Ke,
   its mean and 0xFFFFFFFF).  rtx_debug_light_sample: n seed pairs -> 12 words per seed: light index bits, sample point xyz, s, t (0, 0 for a light without the map), em * tl
   xyz, pdf_l, the seed after the three draws (2); RTX_ERR_STATE for a scene without a light list */
int  rtx_debug_emission(rtx_ctx*, const float* hits4, uint32_t n, float* out8);
int  rtx_debug_light_sample(rtx_ctx*, const uint32_t* seeds2, uint32_t n, float* out12);
/* tests: the device's sampler — n (s, t) pairs -> (r, g, b, 0) — and the device's per-hit albedo — hits4 as rtx_debug_trace_closest writes them -> (Kd' (m.Kd where the
   material has no map), texture id as uint bits or 0xFFFFFFFF); a miss gives (0, 0, 0, 0xFFFFFFFF).  rays8 may be NULL: the albedo depends on the hit record alone */
int  rtx_debug_texture_sample(rtx_ctx*, uint32_t tex, const float* uv2, uint32_t n, float* out4);
int  rtx_debug_albedo(rtx_ctx*, const float* rays8, const float* hits4, uint32_t n, float* out4);
/* tests: the alpha test of the cut-outs, by the device function the traversal runs — hits4 as rtx_debug_trace_closest writes them -> per record (alpha, opacity texture id
   as uint bits); (1.0f, 0xFFFFFFFF) for a miss, for a triangle that is not a cut-out triangle, and for every hit while no cut-out is active */
int  rtx_debug_opacity(rtx_ctx*, const float* hits4, uint32_t n, float* out2);
/* tests: the shading normal of NORMAL MAPS, by the device function k_shade runs — rays8 / hits4 as for rtx_debug_surface -> per record (n'.xyz, normal texture id as uint bits
   or 0xFFFFFFFF: an emitter, a material without a map, no normal map active — n' is then the surface reconstruction's normal); a miss gives (0, 0, 0, 0xFFFFFFFF).
   rtx_debug_tri_tangents: records [first, first + count) of the device's copy of the tangent table, 6 floats each; RTX_ERR_STATE while no normal map is active */
int  rtx_debug_shading_normal(rtx_ctx*, const float* rays8, const float* hits4, uint32_t n, float* out4);
int  rtx_debug_tri_tangents(rtx_ctx*, uint32_t first, uint32_t count, float* out6);
/* ENVIRONMENT LIGHTING (new; the reference's Miss.hlsl:3-11 returns black, so a ray that leaves the scene ends dark and only emissive triangles light anything: an extension,
   unpinned by definition like strategy 3 and map_Kd, pinned by its own definition and properties in tests/test_env_ref.py / tests/test_env.py).  rtx_render and
   rtx_render_adaptive only; rtx_render_v6_pass1 and rtx_render_restir ignore the environment, as they ignore maps and RTX_FLAG_TRANSMISSION.  With no environment bound every
   launch, image, statistic and random-number sequence is what it was.
   DATA.  Per context at most one environment: an N x N OCTAHEDRAL map of linear float32 RGB radiance, 1 <= N <= 2048 (N = 1: the constant sky), row j = v, column i = u, row-major;
   a rotation env_to_world (the 16-float convention above, only the upper 3x3 R is used, its columns orthonormal within 1e-4 else RTX_ERR_INVALID, NULL = identity); a scale,
   finite and >= 0, multiplied into the texels once on the host (float32 product, which must stay finite); flags: RTX_ENV_HIDDEN = primary rays that miss stay black (lighting without
   a visible backdrop).  A texel component that is negative or not finite is RTX_ERR_INVALID.
   MAPPING.  Y is up.  sgn(x) = x >= 0 ? 1 : -1 (so sgn(-0) = 1).  All arithmetic float32 in exactly the written order, no contraction; R[r][c] = env_to_world[c * 4 + r].
   Direction d -> map:
       e.x = (R[0][0] * d.x + R[1][0] * d.y) + R[2][0] * d.z ;  e.y, e.z likewise with R[.][1], R[.][2]                        (e = R^T d)
       s = (|e.x| + |e.y|) + |e.z| ;  q = (e.x / s, e.y / s, e.z / s)
       q.y >= 0 ?  (a, b) = (q.x, q.z)  :  a = (1 - |q.z|) * sgn(q.x), b = (1 - |q.x|) * sgn(q.z)
       u = a * 0.5f + 0.5f ;  v = b * 0.5f + 0.5f
       i = min((int)(u * (float)N), N - 1) ;  j = min((int)(v * (float)N), N - 1) ;  texel t = j * N + i
       r2 = (q.x * q.x + q.y * q.y) + q.z * q.z ;  r3 = r2 * sqrtf(r2)
   Map (u, v) -> direction, the inverse fold:
       a = u * 2 - 1 ;  b = v * 2 - 1 ;  y = (1 - |a|) - |b|
       y < 0 ?  a' = (1 - |b|) * sgn(a), b' = (1 - |a|) * sgn(b)  :  (a', b') = (a, b)
       r2 = (a' * a' + y * y) + b' * b' ;  sr = sqrtf(r2) ;  r3 = r2 * sr ;  inv = 1 / sr ;  q = (a' * inv, y * inv, b' * inv)
       d.x = (R[0][0] * q.x + R[0][1] * q.y) + R[0][2] * q.z ;  d.y, d.z likewise with R[1][.], R[2][.]                        (d = R q)
   On this mapping d_omega = 4 du dv / r^3 with r = |q|, q on the L1 unit sphere (the midpoint sum of 4 / r^3 over a 2048^2 grid is 12.56637061 = 4 pi; r^3 lies in [0.192, 1]),
   so the solid-angle pdf of a direction in texel t is
       pdf = ((pmf[t] * (float)(N * N)) * 0.25f) * r3                                   (r3 of THAT DIRECTION, not of the texel centre)
   Lookup is NEAREST: radiance is constant over a texel, so the pdf follows the radiance exactly up to r3.  Bilinear lookup is not part of this.
   TABLES, built on the host at rtx_commit_scene, in double, sequentially in row-major order, each value rounded to float32 once.  With c = the texel after the scale:
       rc3[j][i]: the inverse fold above in double at (u, v) = ((i + 0.5) / N, (j + 0.5) / N): r2 * sqrt(r2)
       w[j][i] = (((c.r + c.g) + c.b) / 3) / rc3[j][i]
       total = the running sum of w over all texels, row-major from 0 ;  pmf[j][i] = w[j][i] / total
       rowacc[j][i] = the running sum of w[j][0 .. i] from 0 ;  rowsum[j] = rowacc[j][N - 1] ;  acc[j] = acc[j - 1] + rowsum[j] from 0
       conditional[j][i] = rowacc[j][i] / rowsum[j] ;  marginal[j] = acc[j] / total
   and then in each CDF the entries AT AND AFTER the last index with nonzero mass are 2.0f (a row of zero mass: all of its conditional entries).  The device texel is
   (r, g, b, pmf), one 16-byte record: one read gives radiance and pdf.  Selection is "first index with xi < C[index]", the light CDF's binary search: a zero-mass texel is
   never chosen and xi == 1.0f (RandomFloat can return it) lands on the last nonzero one.  An environment whose total weight is 0 has no NEE slot and its misses add zero: such a
   scene runs the kernels and draws the random numbers of the scene without it.
   TRANSPORT.  Environment NEE: ONE extra sample per shaded bounce in NEE slot index nee (after the nee = nee_samples triangle-light samples — 0 without lights —, before the
   continuation).  Four draws in this order: row (marginal), column (that row's conditional), xi_u, xi_v;  u = ((float)i + xi_u) / (float)N, v = ((float)j + xi_v) / (float)N;
   Ln = the direction of (u, v);  L and pmf are the CHOSEN texel's (i, j), r3 the decoded point's, pdf_env as above.  Rejected when dot(normal, Ln) < EPS or not pdf_env > 0.
       mi = pdf_env / (pdf_env + P)   (P = the mixture pdf of Ln: balance heuristic, one sample each) ;  con_k = L_k * (thr_k * F_k) * (cos_x / pdf_env * mi), dropped if not finite or zero
   Shadow ray: origin and tmin of the triangle-light sample, tmax = 10000 (the camera rays' "no limit").  Its rays count in rtx_stats.rays_shadow.
   Miss at bounce b, d = the ray's direction:  b == 0: rad += L(d), or nothing with RTX_ENV_HIDDEN;  b >= 1: mi = prev_pdf / (pdf_env(d) + prev_pdf), mi = 1 when prev_pdf < 0
   (the ray came through a transmission lobe), e_k = (L_k * thr_k) * mi, added if finite.  Triangle-light NEE and the emissive hit are untouched.
   CALLS.  rtx_set_environment with rgb32f == NULL clears the environment (the other arguments are ignored).  Valid before the first commit and on a resident scene; needs
   rtx_commit_scene again (rendering in between is RTX_ERR_STATE).  RTX_ERR_INVALID leaves the scene untouched and committed.  On a resident general scene a commit after this
   call alone uploads tables only: no rebuild, no refit, rtx_stats.bvh_refits and rtx_debug_tree_hash unchanged.  A tiny scene (<= 64 triangles) runs on the general BVH path
   while an environment is bound; the commit that crosses that line, either way, is a rebuild.  With an environment bound rtx_render runs the default separate kernels whatever
   RTX_OPT_FUSED_BVH, RTX_OPT_SHADE_DENSE and RTX_OPT_SORT_MATERIALS say; RTX_OPT_COMPACT_STATE 0 and 1 both work.  rtx_save_scene_cache with an environment bound is
   RTX_ERR_STATE (the file holds none); a loaded cache has no environment.  rtx_denoise is unchanged: misses pass through.  rtx_stats keeps its layout. */
#define RTX_ENV_HIDDEN 1u
int  rtx_set_environment(rtx_ctx*, const float* rgb32f /* N * N * 3; NULL clears */, uint32_t n, const float env_to_world[16] /* NULL = identity */, float scale, uint32_t flags);
/* tests: the device's sampler and lookup, the functions k_shade runs.  RTX_ERR_STATE without a committed environment.
   rtx_debug_env_sample: n seeds (2 uint32 each) -> 12 floats each: world direction(3), pdf, L(3), texel j * N + i as uint bits, the seed after the four draws (2 uint bits), 0, 0
   (RTX_ERR_STATE for an environment without weight: nothing samples it).  rtx_debug_env_eval: n world directions -> 8 floats each: L(3), pdf, texel bits, r3, 0, 0.
   rtx_debug_env_tables: the tables as the device holds them, N * N * 4 | N | N * N floats; any pointer may be NULL */
int  rtx_debug_env_sample(rtx_ctx*, const uint32_t* seeds2, uint32_t n, float* out12);
int  rtx_debug_env_eval(rtx_ctx*, const float* dirs3, uint32_t n, float* out8);
int  rtx_debug_env_tables(rtx_ctx*, float* texels4, float* marginal, float* conditional);
/* CreateAccelerationStructures (Renderer.cpp:893-946) + CollectEmissiveTriangles (:2123-2213) +
   CreateEmissiveTrianglesBuffer (:2237-2280): BVH build, emissive CDF, upload */
int  rtx_commit_scene(rtx_ctx*);
/* SURVEY 8(f3) binary scene cache.  rtx_save_scene_cache writes the committed scene — what the calls above handed over AND what
   rtx_commit_scene derived for the device (MaterialOptimized table + Ess LUTs, compressed 8-wide BVH, leaf-ordered triangles, shading
   records, emissive CDF, tiny-scene records) — to one versioned, checksummed file.  rtx_load_scene_cache REPLACES the context's scene
   by the file's and uploads it (no BVH build: 3.8 M triangles in a fraction of the 2.2 s a commit takes); it returns RTX_ERR_INVALID and
   leaves the current scene untouched for a missing / truncated / corrupt file, another version or another record layout.  The
   reference has no such file (it rebuilds its BLAS / TLAS at start-up, Renderer.cpp:893-946). */
int  rtx_save_scene_cache(rtx_ctx*, const char* path);
int  rtx_load_scene_cache(rtx_ctx*, const char* path);
/* b0 `CameraParams` (UpdateCameraBuffer, Renderer.cpp:1722-1768): view + projection; inverses computed inside */
int  rtx_set_camera(rtx_ctx*, const float view[16], const float proj[16]);
/* THIN LENS (new; the reference's camera is a pinhole: every primary ray starts at viewI[12..14], RayGen_v6_pass1.hlsl:51-95 — an extension, unpinned by definition like the
   environment, pinned by its own definition and properties in tests/test_lens_ref.py / tests/test_lens.py).  Depth of field costs no extra ray: it is another primary ray per
   sample, decided in ray generation.  With no lens set (or radius 0) every launch, image, statistic and random-number sequence is what it was.
   PER PATH.  R = aperture_radius > 0, F = focus_distance, Vi = viewI; (o, d) = the pinhole ray of the path's pixel, computed after the two jitter draws if RTX_FLAG_JITTER is
   set.  All arithmetic float32 in exactly the written order, no contraction; sqrtf and / are IEEE; sincos_ is the one of csrc/rtx_math.hpp:
       xi1 = RandomFloat ;  xi2 = RandomFloat                  (after jitter's draws, before anything of the path: the path starts from the seed state after them)
       r  = sqrtf(xi1) ;  (sn, cs) = sincos_(kTwoPi * xi2)
       lx = (R * r) * cs ;  ly = (R * r) * sn
       cz = |(d.x * Vi[8] + d.y * Vi[9]) + d.z * Vi[10]|        (cosine to the view axis, sign-free: left- and right-handed views alike)
       ft = F / cz
       P.k  = o.k + d.k * ft                                    (k = x, y, z: the point in focus)
       o'.k = (o.k + Vi[0 + k] * lx) + Vi[4 + k] * ly           (the lens point: camera right / up, the first two columns of viewI)
       v = P - o' ;  r2 = (v.x * v.x + v.y * v.y) + v.z * v.z ;  inv = 1.0f / sqrtf(r2) ;  d' = v * inv
   The path starts as (o', d'); if not cz > 0 or a component of d' is not finite it keeps (o, d) — the two draws are consumed either way.  tmin and tmax stay the camera rays'.
   With R = 0 nothing is drawn, the ray is the pinhole ray and the kernels that always ran run.
   WHO SEES IT: rtx_render, rtx_render_adaptive, rtx_debug_primary_rays (which returns (o', d')) and rtx_debug_primary_seeds.  WHO IGNORES IT, keeping the pixel-corner pinhole
   ray as they ignore maps and the environment: rtx_render_v6_pass1, rtx_render_restir, the guides of rtx_denoise, rtx_read_layer's layers 10-17, rtx_focus_distance_at.
   Under a lens the fused tiny-scene path neither shares a pixel's primary hit among its samples (RTX_OPT_SHARED_PRIMARY is ignored) nor culls records per 8x8 block.
   CALLS.  rtx_set_lens is camera state: valid at any time after rtx_create, needs no rtx_commit_scene and never dirties the scene (rtx_stats.bvh_refits and rtx_debug_tree_hash
   unchanged), survives rtx_set_camera, is not part of a scene cache.  NULL = the pinhole.  RTX_ERR_INVALID — a negative or non-finite radius, a focus distance that is not
   finite, or not > 0 while the radius is > 0, a nonzero reserved word — leaves the previous lens in place.  Like a camera move it does not clear the accumulation: that is
   the caller's decision.
   rtx_focus_distance_at is autofocus: it traces the jitter-free pinhole ray of pixel (x, y) of a width x height image exactly as layers 10-17 do (cut-outs and hidden instances
   count) and writes t * cz (a float32 product, cz as above), 0.0f on a miss.  RTX_ERR_STATE before a commit or a camera, RTX_ERR_INVALID for a pixel outside the image. */
typedef struct rtx_lens {
    float    aperture_radius;   /* world units, finite, >= 0; 0 = pinhole (the default) */
    float    focus_distance;    /* world units along the view axis, finite, > 0 (ignored, but still validated as finite, when the radius is 0) */
    uint32_t reserved[2];       /* 0 */
} rtx_lens;
int  rtx_set_lens(rtx_ctx*, const rtx_lens* /* NULL = pinhole */);
int  rtx_focus_distance_at(rtx_ctx*, uint32_t width, uint32_t height, uint32_t x, uint32_t y, float* distance_out);

/* u1 `gPermanentData` RGBA32F W x H (Renderer.cpp:1167-1186): xyz running sum, w sample count.
   rtx_bind_accum lets the caller own the device buffer (W*H*16 bytes, e.g. a torch tensor); NULL = internal. */
int  rtx_bind_accum(rtx_ctx*, void* device_rgba32f, size_t bytes);
int  rtx_clear_accum(rtx_ctx*, uint32_t width, uint32_t height);   /* view-change reset (RayGen_v6_pass3.hlsl:407-423) */
/* 3x DispatchRays (PopulateCommandList, Renderer.cpp:646-673) -> here: the wavefront loop; returns with the frame finished (RTX_OPT_ASYNC on a caller-bound stream: enqueued) */
int  rtx_render(rtx_ctx*, const rtx_params*);
/* ADAPTIVE SAMPLING (new; the reference gives every pixel the same count): rtx_render with a noise threshold and a sample cap instead of a sample count.  rtx_params.spp is
   ignored.  The unit of decision is the 256-slot CHUNK every raygen kernel deals: four 8x8 blocks of one tile, a 32 x 8 pixel strip (with tile_size 16 the whole tile).  A chunk
   is sampled as a whole or not at all.
   State beside u1, cleared by rtx_clear_accum: `half`, a second RGBA32F W x H image holding the running sum of the samples whose id (sample_base + n) is ODD, added in the same
   place and order as u1; per chunk the samples taken and a sticky "converged" flag.  Criterion per valid pixel, float32 in exactly this order, a = u1, h = half, N = a.w:
       d = (|a.x - (h.x + h.x)| + |a.y - (h.y + h.y)|) + |a.z - (h.z + h.z)|          (|sum of the even ids - sum of the odd ids|)
       s = (a.x + a.y) + a.z
       converged = d * d < ((threshold * threshold) * max(s, dark_floor * N)) * N
   A chunk converges when every valid pixel of it has, and is then never sampled again before the next clear.  The comparison is strict: threshold 0 converges nothing and
   gives rtx_render's image of max_spp samples to the bit.  dark_floor 0 means 0.01.  The halves balance at even counts only: min_spp and step_spp must be even and >= 2,
   min_spp <= max_spp (else RTX_ERR_INVALID; a failed call leaves the image untouched).
   One call: chunks without samples get min_spp; then — criterion, list of the chunks neither converged nor at max_spp, its length read back — every listed chunk gets step_spp
   more samples (fewer to land on max_spp), until the list is empty.  A chunk's next sample id is sample_base + its count, seeds depend on pixel and sample id only, and sums
   are added in sample order: the image is a function of the arguments, not of batching, sharding or how the calls were split — a later call with a larger max_spp continues
   where the last one stopped (max 8, then max 16 == max 16 at once, to the bit; keep sample_base).  Shards work as for rtx_render: decisions never look across chunks, and the
   per-chunk state is kept per IMAGE chunk, so one context may also render several shards in turn.  Always synchronous (the host sizes every pass), RTX_OPT_ASYNC or not.
   rtx_stats covers the whole call (rays, paths, kernel_ms summed over the passes; the criterion and list kernels under RTX_K_ADAPT); the per-pixel count is u1's w as ever.
   u1 must hold adaptive samples only: after rtx_render / rtx_render_v6_pass1 / rtx_render_restir, or with another image size or tile_size than the state was begun with,
   the call is RTX_ERR_STATE until rtx_clear_accum.  Path tracer only (no ReSTIR / pass-1 form). */
typedef struct rtx_adaptive {
    uint32_t min_spp, step_spp, max_spp;   /* first pass | later passes | cap, per chunk */
    float    threshold, dark_floor;        /* relative noise of the mean a pixel may keep; floor under sum / N for dark pixels (0 => 0.01) */
    uint32_t reserved[3];                  /* 0 */
} rtx_adaptive;
typedef struct rtx_adaptive_result {
    uint32_t passes;                       /* render passes of this call */
    uint32_t chunks, chunks_converged, chunks_at_max;   /* of this shard, after the call: chunks holding a valid pixel | flagged converged | unconverged at max_spp */
    uint64_t pixel_samples;                /* valid pixel-samples this call added (== rtx_stats.paths) */
} rtx_adaptive_result;
int  rtx_render_adaptive(rtx_ctx*, const rtx_params*, const rtx_adaptive*, rtx_adaptive_result* out /* may be NULL */);
/* DENOISING (new; the reference shows the accumulated mean as it is): an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over the mean of u1, guided by the first
   hit of the pixel-corner primary ray.  u1 is only read: progressive accumulation goes on after a denoise.  The result is a second RGBA32F W x H image (xyz, w = 1.0).
   All arithmetic is float32 in exactly the written order (no contraction); tests/test_denoise_ref.py replays it in numpy and tests/test_denoise.py holds the device to it bit for bit.
   GUIDES per pixel: the ray, tmin and trace of rtx_read_layer's layers 10-17 (pixel corner, jitter-free whatever RTX_FLAG_JITTER says; hidden instances are invisible):
   P = world position, n = shading normal, mat = material id of the surface there.  A pixel is FILTERABLE when the ray hits, mat < material count, no component of that
   material's Ke is > 0 and u1.w > 0; every other pixel (miss, emitter seen directly, no samples) passes through: its output is its input at every level and it contributes to no neighbour.
   INPUT colour c = u1.xyz / max(u1.w, 1).  LEVELS i = 0 .. levels-1, step s = 1 << i, each reading the previous one's output.  For a filterable centre p the taps are
   q = p + s (dx, dy), dy = -2 .. 2 outer, dx = -2 .. 2 inner (row-major, the centre included; the centre is a tap like any other), h = (1/16, 1/4, 3/8, 1/4, 1/16).
   A tap counts if q is inside the image, filterable, and mat_q == mat_p; for a tap that counts
       dn = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z
       wn = max(dn, 0), then wn = wn * wn, normal_power_log2 times
       d  = P_q - P_p
       dp = |(n_p.x*d.x + n_p.y*d.y) + n_p.z*d.z|
       wp = max(1 - dp * inv_sigma_plane, 0)
       dc = (|c_q.x - c_p.x| + |c_q.y - c_p.y|) + |c_q.z - c_p.z|                (this level's input colours)
       wc = max(1 - dc * (inv_sigma_color * s), 0)                               (sigma_color halves per level; * s is exact)
       w  = ((h[dy+2] * h[dx+2]) * wn) * (wp * wc)
       sum.xyz = sum.xyz + w * c_q.xyz ;  sumw = sumw + w                        (sequential, in tap order, from 0)
   and the output is sum.xyz / sumw (the centre tap has wp = wc = 1 and wn = |n|^(2 << normal_power_log2), so sumw > 0).  inv_sigma_* = 1.0f / sigma_*, once, on the host.
   rtx_denoise works on whichever u1 is bound and on the whole image (no shard fields: denoise after rtx_unpack_tiles).  Like rtx_pack_tiles it is synchronous on the context's own
   stream and only ENQUEUES on a caller-bound one, behind a frame that RTX_OPT_ASYNC left in flight, by stream order — unless `out` is given: the counts are read back, which joins
   the stream up to the denoise.  The guides are recomputed by every call (one primary ray per pixel).
   Errors: RTX_ERR_STATE before commit (also: a scene edit not yet committed), camera or any accumulation; RTX_ERR_INVALID for a size other than the accumulation buffer's, for
   levels > 8, normal_power_log2 > 7, a sigma that is negative, not finite or whose reciprocal is not finite, an unknown bit in flags, or a nonzero reserved word.  A failed call leaves u1 and the
   previous denoised image untouched.  rtx_read_denoised* is RTX_ERR_STATE before a successful rtx_denoise and once the accumulation buffer has another size than the denoised image.
   DEFAULT sigma_plane = 2^-6 * the largest extent of the committed scene's bounding box, defined by these float32 operations: for every instance (hidden ones included) and every vertex v
   of its mesh, world_k = ((v.x * m[k] + v.y * m[4+k]) + v.z * m[8+k]) + m[12+k], k = 0, 1, 2, m = the instance's objectToWorld; lo / hi = min / max over all of them;
   extent_k = hi_k - lo_k; sigma_plane = 0.015625f * max(extent).
   MAP GUIDES (opt-in, rtx_denoise_params.flags; with flags == 0 every kernel launched, every buffer allocated and every bit of the result is what it was).  Diffuse texture maps,
   cut-outs and normal maps leave detail INSIDE one material id on geometry that is flat as far as the guides above can tell, and the colour stop alone treats it like noise.  Two
   more guides per pixel, from the same ray, tmin and trace as the guides above (pixel corner, no jitter, no lens; cut-outs and hidden instances count).  For a pixel that is
   filterable by geometry, with hit record (t, u, v, prim), material m and the surface reconstruction sf:
       K  = the Kd' of PER HIT under DIFFUSE TEXTURE MAPS (the value rtx_debug_albedo returns; m.Kd where the material has no map or no map is active)
       A.k = max(K.k, 0.015625f)                                                 (k = x, y, z.  The floor 2^-6 is part of the definition: below it the division would amplify by
                                                                                  more than 64 and the binary16-rounded Kd' gets coarse; the bias it leaves on such a texel is
                                                                                  at most 1/64 of the filtered irradiance)
       nm = the n' of NORMAL-MAPPED HIT with wo = the guide ray's direction negated (sf.normal where no normal map is active or the material has none)
   A pixel that is not filterable by geometry has A = (1, 1, 1) and nm = (0, 0, 0).
   RTX_DENOISE_ALBEDO.  Only FILTERABLE pixels (filterable by geometry and u1.w > 0) are demodulated.  Level 0's input colour of such a pixel is
       c.k = (u1.k / max(u1.w, 1)) / A.k                                         (two IEEE divisions, in this order)
   every level then runs as defined above on those colours, and the LAST level's output of such a pixel is
       o.k = (sum.k / sumw) * A.k
   Every other pixel passes through exactly as without the flag: its output is its input, to the bit, at every level; a tap never reads such a pixel, so the two domains never mix.
   RTX_DENOISE_MAPPED_NORMALS.  Only the normal stop changes: dn = (nm_p.x*nm_q.x + nm_p.y*nm_q.y) + nm_p.z*nm_q.z.  The plane stop keeps n_p of the guides above: a perturbed
   normal must not make a flat wall leave its own tangent plane.
   CONSEQUENCES.  With no normal map active RTX_DENOISE_MAPPED_NORMALS gives the bits of flags == 0 (nm == n to the bit), and so does a scene whose normal maps hold only flat
   texels.  RTX_DENOISE_ALBEDO changes no pass-through pixel.  Without jitter and without a lens every sample of a pixel hits the guide's texel, so A is the samples' own albedo;
   under RTX_FLAG_JITTER or a lens it is the pixel-corner ray's albedo (documented, not corrected).  Specular, metallic and roughness terms are not demodulated.
   tests/denoise_maps_ref.py replays both in numpy; tests/test_denoise_maps.py holds the device to it bit for bit. */
#define RTX_DENOISE_ALBEDO         1u
#define RTX_DENOISE_MAPPED_NORMALS 2u
typedef struct rtx_denoise_params {
    uint32_t levels;              /* 1..8; 0 => 5 */
    uint32_t normal_power_log2;   /* 1..7; 0 => 5 (cos^32) */
    float    sigma_color;         /* > 0; 0 => 0.5 */
    float    sigma_plane;         /* world units, > 0; 0 => 2^-6 * largest extent of the committed scene's bounding box */
    uint32_t flags;               /* RTX_DENOISE_* (MAP GUIDES above); 0 = the filter as it always was; any other bit is RTX_ERR_INVALID */
    uint32_t reserved[3];         /* 0 */
} rtx_denoise_params;
typedef struct rtx_denoise_result {
    uint32_t levels;
    uint32_t pixels_filtered;
    uint32_t pixels_passed;
    double   guides_ms;           /* hipEvent, 0 unless RTX_OPT_KERNEL_TIMING */
    double   filter_ms;           /* hipEvent, 0 unless RTX_OPT_KERNEL_TIMING */
} rtx_denoise_result;
int  rtx_denoise(rtx_ctx*, uint32_t width, uint32_t height, const rtx_denoise_params* /* NULL = all defaults */, rtx_denoise_result* /* may be NULL */);
int  rtx_read_denoised(rtx_ctx*, float* rgba32f, size_t bytes);
int  rtx_read_denoised_srgb8(rtx_ctx*, uint8_t* rgba8, size_t bytes);   /* k_srgb8 over the denoised image */
/* the guides as the filter reads them: per pixel P3, material word as uint bits (0xFFFFFFFF = not filterable by geometry; P and n are then 0), n3, 0 */
int  rtx_debug_denoise_guides(rtx_ctx*, uint32_t width, uint32_t height, float* out8 /* W*H*8 */);
/* the MAP GUIDES as the filter reads them under a flag: per pixel A3, 0, nm3, 0 ((1, 1, 1, 0, 0, 0, 0, 0) where the pixel is not filterable by geometry); errors as above */
int  rtx_debug_denoise_map_guides(rtx_ctx*, uint32_t width, uint32_t height, float* out8 /* W*H*8 */);
/* DENOISING, VARIANCE-GUIDED (rtx_denoise_variance; rtx_denoise and its struct are unchanged).  The same filter, guides, taps, wn and wp, but the colour stop is scaled by the
   centre pixel's OWN noise instead of one constant for the image (after Schied et al. 2017, SVGF): rtx_render_adaptive keeps `half`, the running sum of the odd sample ids, and
   with u1 that gives an unbiased per-pixel estimate of the variance of the mean.  All arithmetic is float32 in exactly the written order, no contraction, IEEE / and sqrtf;
   tests/denoise_var_ref.py replays it in numpy and tests/test_denoise_var.py holds the device to it bit for bit.
   a = u1, hb = `half`.  Filterable, the taps, h[], wn, wp, A and nm are exactly as in DENOISING and MAP GUIDES above.
   LEVEL-0 INPUT of a pixel with a.w > 0:
       cnt = max(a.w, 1);   c.k = a.k / cnt;   e.k = (a.k - (hb.k + hb.k)) / cnt             (k = x, y, z; e = (even sum - odd sum) / N)
       under RTX_DENOISE_ALBEDO, filterable pixels only:   c.k = c.k / A.k;   e.k = e.k / A.k
       el = (0.2126f * e.x + 0.7152f * e.y) + 0.0722f * e.z;   v = el * el                    (unbiased for the variance of the mean's luminance when the halves balance)
   EVERY LEVEL i, step s = 1 << i, for a filterable centre p, reading this level's input (c, v):
       prefilter: q = p + (dx, dy), dy = -1 .. 1 outer, dx = -1 .. 1 inner, ALWAYS one pixel apart whatever s; g = (1/16, 1/8, 1/16, 1/8, 1/4, 1/8, 1/16, 1/8, 1/16);
                  a position counts under the taps' rule (inside the image, filterable, mat_q == mat_p):   sg = sg + g * v_q;   sgw = sgw + g      (sequential from 0)
       gv  = sg / sgw
       inv = 1.0f / (sigma_var * sqrtf(gv) + 9.5367431640625e-07f)                            (2^-20: part of the definition; it bounds inv where a pixel's halves agree)
       l_p = (0.2126f * c_p.x + 0.7152f * c_p.y) + 0.0722f * c_p.z;   l_q likewise
       the 25 taps, same order and counting rule, wn and wp unchanged (nm under RTX_DENOISE_MAPPED_NORMALS):
           dl = |l_q - l_p|;   wc = max(1 - dl * inv, 0);   w = ((h[dy+2] * h[dx+2]) * wn) * (wp * wc)
           sum.xyz = sum.xyz + w * c_q.xyz;   sumw = sumw + w;   sumv = sumv + (w * w) * v_q
       output c = sum.xyz / sumw,   v = sumv / (sumw * sumw)
   Pass-through pixels behave as in rtx_denoise: their output is their input at every level, and they contribute to no tap and to no prefilter.  Under RTX_DENOISE_ALBEDO the
   last level multiplies by A.  The last level stores w = 1.0; the filtered variance is not part of the result.  There is no sigma_color: the variance shrinks level by level,
   which replaces Dammertz's halving.  The result is the denoised image of rtx_denoise (rtx_read_denoised, rtx_read_denoised_srgb8); stream semantics and the result fields are
   rtx_denoise's.
   STATE.  The call needs the adaptive state that belongs to u1: every sample since the last clear came from rtx_render_adaptive, the state is laid out for this width and
   height, and every one of those calls was unsharded (shard_count <= 1; rtx_unpack_tiles counts as sharded: `half` is not gathered).  Anything else is RTX_ERR_STATE, on top
   of rtx_denoise's own state errors.  A fixed sample count is rtx_render_adaptive with threshold 0, which is rtx_render's image to the bit.  RTX_ERR_INVALID as rtx_denoise:
   size, levels, power, a sigma that is negative, not finite or whose reciprocal is not finite, unknown flag bits, a nonzero reserved word.  A failed call leaves u1, `half` and
   the previous denoised image untouched. */
typedef struct rtx_denoise_var_params {
    uint32_t levels;              /* 1..8; 0 => 5 */
    uint32_t normal_power_log2;   /* 1..7; 0 => 5 */
    float    sigma_var;           /* > 0: standard deviations of the pixel's own noise at which the colour stop reaches zero; 0 => 4 (Schied et al. 2017, sigma_l) */
    float    sigma_plane;         /* as rtx_denoise_params */
    uint32_t flags;               /* RTX_DENOISE_ALBEDO | RTX_DENOISE_MAPPED_NORMALS, same meaning; any other bit is RTX_ERR_INVALID */
    uint32_t reserved[3];         /* 0 */
} rtx_denoise_var_params;         /* 32 bytes */
int  rtx_denoise_variance(rtx_ctx*, uint32_t width, uint32_t height, const rtx_denoise_var_params* /* NULL = defaults */, rtx_denoise_result* /* may be NULL */);
int  rtx_read_adaptive_half(rtx_ctx*, float* rgba32f, size_t bytes);     /* copy of `half` to the host, like rtx_read_accum; RTX_ERR_STATE without the state above */
/* (v, gv) of level 0 as the filter reads them (flags: RTX_DENOISE_ALBEDO divides by A; the normals do not enter); (0, 0) for a pixel that is not filterable; state as above */
int  rtx_debug_denoise_variance(rtx_ctx*, uint32_t width, uint32_t height, uint32_t flags, float* out2 /* W*H*2 */);
/* The reference's OWN first pass, literally: RayGen of RayGen_v6_pass1.hlsl:48-190 (first DispatchRays,
   Renderer.cpp:651-654): primary hit, SampleRIS (Sampler_v6.hlsl:653-736), visibility, SamplePathSimple
   (Path_Sampler_v6.hlsl:3-286).  params: nee_samples = nee_samples_DI = nee_samples (Common_v6.hlsl:8-9, reference 4),
   max_bounces = `bounces` (:11, reference 3), spp samples are run one after the other; sdata.debug (or L1 on emissive
   primary hits) is added to u1.  The pass-1 outputs u2 `g_Reservoirs_current` / u4 `g_Reservoirs_current_gi` (40 B) and
   u6 `g_sample_current` (60 B) keep the last sample, in MapPixelID order (Common_v6.hlsl:173-198). */
int  rtx_render_v6_pass1(rtx_ctx*, const rtx_params*);
size_t rtx_pass1_slots(uint32_t width, uint32_t height);            /* records per buffer: ceil(w/4)*ceil(h/4)*16 */
int  rtx_read_pass1_buffers(rtx_ctx*, void* reservoirs_di40, void* reservoirs_gi40, void* samples60, size_t slots);
/* The reference's full frame: pass 1, then RayGen2 = temporal reuse (RayGen_v6_pass2.hlsl:46-204, second DispatchRays,
   Renderer.cpp:662-664) and RayGen3 = spatial reuse + final shade (RayGen_v6_pass3.hlsl:46-441, third DispatchRays, :671-673)
   with the pairwise MIS of MIS_v6.hlsl / MIS_GI_v6.hlsl.  `spp` = number of consecutive frames (frame_seed, frame_seed+1, ...)
   rendered with the current camera; each adds ReconnectDI*W + f_gi*W_gi to u1.  u3/u5/u7 (`g_*_last`) persist in the context
   between calls; rtx_set_camera keeps the previous view/projection for the reprojection; rtx_restir_reset zeroes the history.
   ON SHARDS (shard_count > 1; one frame per call: spp = 1): passes 1 and 2 run on the shard's tiles dilated by the 20-px radius of the spatial pass (the
   halo is recomputed, seeds depend on the pixel only), pass 3 and the accumulation on the shard's own tiles; between frames the shards exchange the history of
   their own tiles — rtx_restir_pack_state -> ONE all-gather (140 B per pixel) -> rtx_restir_unpack_state — because the temporal pass reprojects to arbitrary
   pixels.  Images and histories are bit-identical to the unsharded run. */
int  rtx_render_restir(rtx_ctx*, const rtx_params*);
int  rtx_restir_state_slab_bytes(const rtx_params*, size_t* bytes_per_shard);
int  rtx_restir_pack_state(rtx_ctx*, const rtx_params*, void* device_slab);                       /* u3 / u5 / u7 of my tiles -> slab */
int  rtx_restir_unpack_state(rtx_ctx*, const rtx_params*, const void* device_slabs_all_shards);   /* all shards' slabs -> my u3 / u5 / u7 */
/* HALO EXCHANGE of the history ("halo exchange (20 px) if tiles are sharded"; round 5) — instead of all-gathering every rank's 140 B per pixel (326 MB received
   per rank and frame at 1080p on 8 ranks), a rank of the RTX_FLAG_BLOCK_TILES deal sends each neighbour only the part of its own rectangle that lies within `halo_px` of the
   neighbour's rectangle, and receives the mirror image: <= 8 peers (point-to-point, one xGMI link each), ~10 MB sent per rank.  What makes it sufficient: passes 1 + 2 of the
   next frame run on the rank's rectangle dilated by the 20-px radius of the spatial pass, and the temporal pass reads the history at the REPROJECTED pixel — so the history must
   be valid in the rectangle dilated by 20 px + the largest reprojection displacement of a frame, i.e. halo_px >= 20 + that displacement (32 = one tile edge of the sharded deal
   covers 12 px of motion per frame).  The context KNOWS where its history is valid (own rectangle after a frame, + halo_px after rtx_restir_unpack_halo, the whole image after
   rtx_restir_unpack_state / rtx_restir_reset) and COUNTS every temporal read that lands outside it: rtx_stats.restir_stale_history_reads of the frame must be 0 — a caller that
   sees it rise (a camera cut) falls back to the all-gather (rtx_restir_pack_state / unpack_state) and repeats the frame.  With the count at 0, images and the history inside
   the valid region are bit-identical to the unsharded run.
   rtx_restir_halo_plan needs no context (message via rtx_last_error(NULL)): peers in ascending rank order, regions as pixel rectangles [x0, x1) x [y0, y1), records in
   row-major order, 140 B each (Reservoir_DI 40 | Reservoir_GI 40 | SampleData 60), offsets into ONE send and ONE receive buffer per rank.  send region of (me -> q) ==
   receive region of (q <- me) by construction (tests/test_multigpu_gloo.py pins the symmetry). */
typedef struct rtx_halo_peer {
    uint32_t rank;
    uint32_t send_x0, send_y0, send_x1, send_y1;     /* part of MY rectangle within halo_px of the peer's */
    uint32_t recv_x0, recv_y0, recv_x1, recv_y1;     /* part of the PEER's rectangle within halo_px of mine */
    uint64_t send_offset, send_bytes, recv_offset, recv_bytes;
} rtx_halo_peer;
int  rtx_restir_halo_plan(const rtx_params*, uint32_t halo_px, rtx_halo_peer* peers, uint32_t max_peers, uint32_t* npeers, uint64_t* send_bytes_total, uint64_t* recv_bytes_total);
int  rtx_restir_pack_halo(rtx_ctx*, const rtx_params*, uint32_t halo_px, void* device_send_buffer);            /* u3 / u5 / u7 of every send region -> send buffer (enqueued) */
int  rtx_restir_unpack_halo(rtx_ctx*, const rtx_params*, uint32_t halo_px, const void* device_recv_buffer);    /* receive buffer -> my u3 / u5 / u7; the history is valid in my rectangle + halo_px afterwards */
int  rtx_restir_reset(rtx_ctx*);
int  rtx_read_restir_last(rtx_ctx*, void* reservoirs_di40, void* reservoirs_gi40, void* samples60, size_t slots);   /* u3 / u5 / u7 */
int  rtx_read_accum(rtx_ctx*, float* rgba32f, size_t bytes);       /* copy of u1 to the host */
/* u0 `gOutput` layer 0, RGBA8 UNORM after sRGB OETF (RayGen_v6_pass3.hlsl:405,428-441; Common_v6.hlsl:353-376) */
int  rtx_read_srgb8(rtx_ctx*, uint8_t* rgba8, size_t bytes);
/* u0 `gOutput` is a 30-layer RGBA8 array and 'C' cycles the displayed layer through m_displayLevels = {0, 10..17, 20..28} (Renderer.h:298-299,
   Renderer.cpp:690-698, 748-754).  The reference's live shaders only write layer 0.  Here: 0 = the image, 10-17 = first-hit debug attributes of the
   pixel-corner primary ray (10 normal, 11 depth, 12 material id, 13 Kd, 14 instance id, 15 barycentrics, 16 Ke, 17 roughness / metallic / dissolve;
   defined in csrc/rtx_k_film.hpp: k_debug_layer), every other layer < 30 opaque black. */
int  rtx_read_layer(rtx_ctx*, uint32_t layer, uint32_t width, uint32_t height, uint8_t* rgba8, size_t bytes);
int  rtx_get_stats(rtx_ctx*, rtx_stats* out);
/* t6 `g_EmissiveTriangles` as built by rtx_commit_scene (80 B records, Renderer.h:113-124) */
int  rtx_get_lights(rtx_ctx*, void* out80, uint32_t max_count, uint32_t* count_out);

/* multi-GPU (new; the reference is single-GPU): owned tiles of the accumulation buffer <-> compact
   [tiles_per_shard][tile_size^2] float4 slab for one RCCL (all)gather.  Pointers are DEVICE pointers.
   On the context's own stream both calls are synchronous; on a caller-bound stream (rtx_set_stream) they only enqueue, so that
   pack -> collective -> unpack runs stream-ordered without a host round trip (a 1/8-shard frame is ~2.7 ms). */
int  rtx_shard_slab_bytes(const rtx_params*, size_t* bytes_per_shard);
int  rtx_pack_tiles(rtx_ctx*, const rtx_params*, void* device_slab);
int  rtx_unpack_tiles(rtx_ctx*, const rtx_params*, const void* device_slabs_all_shards);

/* kernel-level entry points used by the parity tests (host arrays in/out; run the SAME device kernels
   the render loop uses).  rays8 = (ox,oy,oz,tmin, dx,dy,dz,tmax) per ray.
   hits4 = (t,u,v, global triangle id as uint bits; 0xFFFFFFFF = miss) — TraceRay closest hit, a11. */
int  rtx_debug_primary_rays(rtx_ctx*, const rtx_params*, uint32_t sample_id, float* rays8 /* W*H*8 */);
/* ... and the seed state (s0, s1) those paths start from: after RTX_FLAG_JITTER's two draws and the lens's two (THIN LENS above) */
int  rtx_debug_primary_seeds(rtx_ctx*, const rtx_params*, uint32_t sample_id, uint32_t* seeds2 /* W*H*2 */);
int  rtx_debug_trace_closest(rtx_ctx*, const float* rays8, uint32_t n, float* hits4);
int  rtx_debug_trace_any(rtx_ctx*, const float* rays8, uint32_t n, uint8_t* occluded);
/* closest-hit traversal of the BVH (never the tiny-scene path) that reports its work: stats4 = n * (t, node steps, triangle tests,
   prim bits) — tree-quality measurements for DESIGN.md, not part of the reference boundary */
int  rtx_debug_trace_stats(rtx_ctx*, const float* rays8, uint32_t n, float* stats4);
/* RTX_OPT_TRACE_COUNTERS: node steps / triangle tests of the closest-hit rays and of the any-hit rays traced by the persistent kernels since the last call (which resets them) */
int  rtx_debug_trace_counters(rtx_ctx*, uint64_t out4[4]);
/* downloads the resident wide BVH and checks it on the host: 0 = every triangle is in exactly one leaf slot and inside all the
   decoded boxes above it (what the GPU refit must preserve); > 0 = validator code; < 0 = RTX_ERR_*.  Triangles of hidden instances (rtx_set_instance_visible; e1.w = +inf)
   must be exactly those of the instances committed as hidden, still sit in their leaf slot, are exempt from containment and must not widen any box */
int  rtx_debug_validate_bvh(rtx_ctx*);
/* FNV-1a hashes of the wide tree as the device holds it: out[0] the node records, out[1] the leaf-ordered triangle records — two contexts hold the same tree iff both agree
   (the GPU build against its host twin, a loaded scene cache against the build it was saved from) */
int  rtx_debug_tree_hash(rtx_ctx*, uint64_t out2[2]);
/* tree quality after refits (tooling, and what RTX_OPT_DEFORM_REBUILD >= 2 decides by): the sum over the wide nodes of half-area(node box) / half-area(root box) — the expected
   number of node visits of a random line — out2[0] as the tree is now, out2[1] right after its last build.  Reproducible to the bit.  RTX_ERR_STATE for a tree the GPU refit
   does not handle (tiny scenes).  A host-built tree that was never refitted is refitted here once (unchanged geometry) to get its boxes */
int  rtx_debug_tree_cost(rtx_ctx*, double out2[2]);
/* the wide tree itself (tooling: diffing two trees that should be equal): which = 0 the device's records, 1 the host builder's mirror of them (RTX_ERR_STATE when the tree was
   built on the device).  nodes: rtx_stats.bvh_nodes x 80 bytes, tris: rtx_stats.bvh_refs x 48 bytes; either may be NULL */
int  rtx_debug_read_tree(rtx_ctx*, int which, void* nodes, uint64_t nodes_bytes, void* tris, uint64_t tris_bytes);
/* what the HOST builder keeps between commits for its refits (tooling): the binary tree (64-byte records) and the leaf order (uint32 per leaf reference).  In: the capacities
   of the two buffers, out: the sizes in bytes; a buffer that is too small (or NULL) is left alone */
int  rtx_debug_read_host_build(rtx_ctx*, void* nodes2, uint64_t* nodes2_bytes, void* leaf_order, uint64_t* leaf_order_bytes);
/* FNV-1a hashes of what the host side holds between commits (tooling: which call changed something it should not have): {mesh indices, mesh vertices, material ids +
   materials, instance records, leaf order, binary tree, wide tree mirror, shade records + object-space triangles + leaf slots} */
int  rtx_debug_host_checksums(rtx_ctx*, uint64_t out8[8]);
/* the last geometry-changing rtx_commit_scene: ms5 = {GPU build: boxes + keys, sort, PLOC rounds, top of the tree on the host, layout} (all 0 after a host build),
   counts4 = {wide nodes, leaf entries, PLOC rounds, clusters handed to the host} */
int  rtx_debug_build_info(rtx_ctx*, double ms5[5], uint32_t counts4[4]);
/* out16 per hit = pos3, matID bits, normal3, area, inst bits, flat3, pad4 (ClosestHit, Hit_v6.hlsl:12-61) */
int  rtx_debug_surface(rtx_ctx*, const float* rays8, const float* hits4, uint32_t n, float* out16);
/* in9 = n(3) wo(3) wi(3); out8 = f(3), pdf, p_d, p_s, 0, 0 */
int  rtx_debug_bsdf_eval(rtx_ctx*, uint32_t mat_id, uint32_t flags, const float* in9, uint32_t n, float* out8);
/* in8 = n(3) wo(3) seed(2 uint bits); out8 = wi(3), strategy bits, seed_out(2), 0, 0 */
int  rtx_debug_bsdf_sample(rtx_ctx*, uint32_t mat_id, uint32_t flags, const float* in8, uint32_t n, float* out8);
/* TEA RNG on the device: n draws from one seed (Common_v6.hlsl:119-138) */
int  rtx_debug_tea(rtx_ctx*, uint32_t seed[2], uint32_t n, float* out);

#ifdef __cplusplus
}
#endif
#endif

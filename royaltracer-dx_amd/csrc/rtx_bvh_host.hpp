// rtx_bvh_host.hpp — the host-side BVH code: the binary builder (rtx_bvh_build.cpp), the wide collapse and the tree validators (rtx_bvh_wide.cpp), the replay of the
// device traversal (rtx_bvh_replay.cpp).  Included by rtx_scene_host.hpp, which holds BuiltScene.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <stdint.h>
#include "rtx_types.hpp"

namespace rtx {

struct BuiltScene;

// Knobs of the BVH builder (defaults = what the product builds; tools/bvh_lab.cpp and the A/B tools change them by key).
struct BvhBuildOptions {
    int      bins = 16;           // binned SAH: bins per axis for nodes above `sweep_below`
    uint32_t sweep_below = 0;     // nodes with at most this many references use the full-sweep SAH (every centroid position) instead of bins
    uint32_t leaf_stop = 1;       // nodes with at most this many references are not split further (the wide collapse merges small subtrees into leaf slots anyway).  1 since round 5:
                                  // chosen on the HARD stand-ins (profiles/r05_bvh_lab.md: closest-hit cost -2.1 % / -2.8 %, any-hit -1.1 % / -0.7 %; nothing on the uniform ones)
    double   split_alpha = 0.0;   // spatial splits where the object split's two sides overlap by more than this fraction of the scene's surface area (0 = never)
    double   split_budget = 0.3;  // ... and at most this many extra references, as a fraction of the triangle count
    int      reinsert_passes = 2; // passes of the insertion-based topology optimisation
    double   reinsert_frac = 1.0; // share of the nodes (largest boxes first) a pass tries to re-insert ...
    uint32_t reinsert_cap = 200000; // ... and at most this many of them
    int      slot_assign = 0;     // collapse_bvh8: children to octant slots greedily (0) or by the exact maximum of the summed diagonal projections (1)
    double   tri_cost = 0.7;      // collapse_bvh8: cost of a triangle test relative to a node step
    int      threads = 0;         // build_bvh: threads of the top-down phase (0 = up to 16 of the machine's; 1 = serial).  The tree does not depend on it
    int      ploc_radius = 0;     // > 0: the bottom-up PLOC builder with this search radius below the top-down SAH builder (the host twin of the GPU build, csrc/rtx_build.hip)
    uint32_t ploc_top = 16384;    // ... which stops at this many clusters; the SAH builder (+ re-insertion) then builds the top of the tree over them (1: PLOC to the root)
};
BvhBuildOptions& bvh_build_options();                      // process-wide defaults: what a new SceneHost starts with (RTX_BVH="key=value,..." in the environment edits them once)
bool bvh_build_option(const char* key, double value);      // edits the defaults; false: unknown key
bool bvh_build_option(BvhBuildOptions& o, const char* key, double value);

// tooling: RTX_BUILD_TIMES=1 prints the phases of a commit to stderr (tools/bvh_lab, tools/build_time.py): lap(name) = the time since the last lap
struct BuildStopwatch {
    const char* prefix; int width; bool on; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    BuildStopwatch(const char* prefix_, int width_, bool on_ = getenv("RTX_BUILD_TIMES") != nullptr) : prefix(prefix_), width(width_), on(on_) {}
    void lap(const char* what) {
        if (!on) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "%s%-*s %.3f s\n", prefix, width, what, std::chrono::duration<double>(t - t0).count());
        t0 = t;
    }
};

// ---- rtx_bvh_build.cpp ----
// binned-SAH BVH2 over world-space triangles (9 floats each); fills nodes (breadth-first, children boxes in
// parent) and the leaf-ordered triangle permutation.
void refit_bvh(const std::vector<float>& wtri, float pad_abs, std::vector<NodeGPU>& nodes, const std::vector<uint32_t>& leaf_order);
void build_bvh(const std::vector<float>& wtri, float pad_abs, std::vector<NodeGPU>& nodes,
               std::vector<uint32_t>& leaf_order, uint32_t& max_depth, const BvhBuildOptions& opt = bvh_build_options());
// the top of a PLOC tree over m cluster boxes (mn.xyz, mx.xyz each): top-down SAH + re-insertion, root first; child >= 0: node index, < 0: ~cluster (host twin and GPU build share it)
struct ClusterTopNode { float mn[3], mx[3]; int32_t left, right; };
void build_cluster_top(const float* boxes6, uint32_t m, const BvhBuildOptions& opt, std::vector<ClusterTopNode>& out);

// ---- rtx_bvh_wide.cpp ----
// collapse the binary tree into the compressed 8-wide device form (largest-area internal child opened first, octant-ordered
// slots, outward-rounded byte quantisation); tri_slots = leaf-order slots in the wide tree's triangle order; max_stack =
// bound on the sibling-group entries a traversal can hold (one per level).  Returns false on a malformed input tree.
bool collapse_bvh8(const std::vector<NodeGPU>& nodes2, std::vector<Node8GPU>& nodes8, std::vector<uint32_t>& tri_slots, uint32_t& max_stack,
                   std::vector<uint32_t>* level_start = nullptr, const BvhBuildOptions& opt = bvh_build_options());
// the leaf triangle of global triangle g from its nine world-space floats: v0 (w = id bits), e1 (w = the hit definition's determinant floor, rtx_math.hpp), e2
inline TriGPU leaf_triangle(const float* t, uint32_t g) {
    const f3 v0 = mk3(t[0], t[1], t[2]);
    const f3 e1 = mk3(t[3], t[4], t[5]) - v0, e2 = mk3(t[6], t[7], t[8]) - v0;
    return TriGPU{{v0.x, v0.y, v0.z, u2f(g)}, {e1.x, e1.y, e1.z, tri_det_floor(e1, e2)}, {e2.x, e2.y, e2.z, 0.0f}};
}
void leaf_triangles(const std::vector<float>& wtri, const std::vector<uint32_t>& leaf_order, std::vector<TriGPU>& tris);      // tris[s] = leaf_triangle of leaf_order[s]
// binary tree -> device traversal form: B.nodes, B.tris (leaf order) -> B.nodes8, B.tri_slots8, B.stack8, B.level_start8 and B.tris8 = B.tris in the wide tree's order.
// Derived data, redone after a refit too (O(nodes)).  false: collapse_bvh8 refused the tree
bool wide_from_binary(BuiltScene& B, const BvhBuildOptions& opt = bvh_build_options());
// coverage check of a wide tree on its DECODED boxes (tests, rtx_debug_validate_bvh): 0 = children follow parents, every leaf slot entry order[tri_slots[i]] is a
// triangle, and every triangle is COVERED: referenced once and inside all boxes above that reference, or — a triangle a spatial split handed to several leaves —
// each of a fixed set of 28 points on it (corners, edge thirds, interior lattice) lies inside all boxes above one of its references; otherwise a small positive code.
// hidden (optional, one flag per leaf entry; rtx_set_instance_visible): a hidden entry must still sit in exactly one leaf slot but is exempt from containment, and it must
// not widen any box: a child without visible content is quantised empty (near byte 255, far byte 0 on every axis: code 25 otherwise), every other child's decoded box
// exceeds the bounds of the visible triangles below it by no more than the leaf padding pad_abs, two steps of the node's byte grid and float rounding (code 26)
struct CoverCheck {                                         // coverage bookkeeping of the tree validators
    struct Part { uint32_t tri; double b[6]; };
    const std::vector<float>& w; std::vector<uint32_t> refs; std::vector<Part> boxes;
    explicit CoverCheck(const std::vector<float>& world_tris9);
    void count(uint32_t tri);                                // first pass: one call per reference
    int add(uint32_t tri, const double mn[3], const double mx[3]);   // second pass: the box chain above a reference (intersection of all boxes above it)
    int finish();
};
int validate_bvh8(const std::vector<float>& world_tris9, const std::vector<Node8GPU>& nodes, const std::vector<uint32_t>& order,
                  const std::vector<uint32_t>& tri_slots, uint32_t* max_stack_seen, const std::vector<uint8_t>* hidden = nullptr, double pad_abs = 0.0);

// ---- rtx_bvh_replay.cpp ----
// host-side replay of the device traversal on B.nodes8 / B.tris8 (counts for tools/bvh_lab.cpp and the any-hit probe)
struct ReplayHit { float t; uint32_t slot, prim; uint32_t steps, tris; };     // prim = global triangle id or 0xffffffff; steps = node steps, tris = triangle tests
ReplayHit replay_trace(const BuiltScene& B, const float o[3], const float d[3], float tmin, float tmax, bool any, uint32_t any_order = 0, float t_known = -1.0f,
                       std::vector<uint8_t>* seq = nullptr);      // seq: per node step, the number of triangles it queued (tools/bvh_lab: wave-schedule simulation)
bool replay_tri_test(const float o[3], const float d[3], const TriGPU& Tg, float tmin, float tmax, float& t);     // the replay's triangle test alone (tools/soup_lab.cpp: brute force in the same arithmetic)
uint32_t probe_anyhit_order(const BuiltScene& B);

}  // namespace rtx

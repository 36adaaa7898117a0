// rtx_refit.hip — the commit path's kernels: GPU refit of the wide BVH and the tree-cost measure, with their launchers (declared in rtx_kernels.hpp).
// A translation unit of its own: it needs rtx_math.hpp and kBlock, nothing of the traversal or shading headers and none of the tooling globals.
#include <hip/hip_runtime.h>
#include "rtx_kernels.hpp"
#include "rtx_dev_common.hpp"   // kBlock

namespace rtx {

// GPU refit of the wide BVH after a transform-only commit (the reference refits its TLAS every frame: Renderer.cpp:594,
// TopLevelASGenerator.cpp:149-250).  Topology, slot assignment and triangle order stay; k_refit_tris re-derives the world-space
// triangles from the object-space vertices with the host's operation order (xform_point: bit-identical TriGPU records, so the
// triangle tests still match the oracle's), k_refit_nodes re-derives and re-quantises the child boxes level by level, deepest
// first.  Quantisation is conservative by construction: lo - p is rounded DOWN before floor(), hi - p UP before ceil(), and
// 2^e is chosen with 255 * 2^e >= extent, so the decoded planes bracket the float boxes exactly as the host's double-checked
// build does.
// ---------------------------------------------------------------------------------------------
// directed-rounding stand-ins (HIP has no __fsub_rd / __fsub_ru here): the neighbours of the round-to-nearest result bracket the
// exact difference (|exact - fl| <= half a spacing), at the price of at most one extra spacing of slack
__device__ __forceinline__ float next_below(float x) { uint32_t b = f2u(x); if (x > 0.0f) b--; else if (x < 0.0f) b++; else b = 0x80000001u; return u2f(b); }
__device__ __forceinline__ float next_above(float x) { uint32_t b = f2u(x); if (x > 0.0f) b++; else if (x < 0.0f) b--; else b = 0x00000001u; return u2f(b); }
__device__ __forceinline__ float sub_down(float a, float b) { return next_below(a - b); }
__device__ __forceinline__ float sub_up(float a, float b) { return next_above(a - b); }

// PARTIAL refit (round 4): `moved` != nullptr names the instances whose transform changed since the last commit.  Only their triangles are re-derived (tri_dirty[s] says
// which leaf entries those were), and k_refit_nodes re-quantises only nodes with a dirty triangle or a dirty child (node_dirty), taking the float box of a clean child
// from node_aabb, which the previous refit left there.  A frame that moves one small instance of a large scene (the reference's own loop: Renderer.cpp:444-452) then costs
// the launches, not the scene.  The padding scale only grows in a partial refit (the untouched boxes keep the padding they were built with: still conservative).
// INSTANCE VISIBILITY (rtx_set_instance_visible): `hidden` != nullptr names the instances that no ray may see.  A triangle of such an instance keeps its true world-space
// record — same operations, same bits — except e1.w, the determinant floor, which becomes +inf: the first comparison of tri_test / tri_test_flat, |det| > e1.w, then fails for
// every ray (finite or NaN det), with no instruction added to any traversal kernel.  That record is all correctness rests on; k_refit_nodes below reads the same marker to
// leave the triangle out of every box, so that rays do not pay for it either.  A hidden triangle does not feed the padding scale.
// VIS = false is the instantiation of scenes with nothing hidden: the kernels as they were before visibility existed, instruction for instruction.
template <bool VIS>
__global__ __launch_bounds__(kBlock) void k_refit_tris(TriGPU* __restrict__ tris, uint32_t ntris, const TriShade* __restrict__ shade, const InstGPU* __restrict__ insts,
                                                       const F4* __restrict__ objtris, uint32_t* __restrict__ scale_bits, const uint32_t* __restrict__ moved, uint8_t* __restrict__ tri_dirty,
                                                       const uint32_t* __restrict__ hidden) {
    __shared__ uint32_t s_max;
    if (threadIdx.x == 0) s_max = 0;
    __syncthreads();
    const uint32_t s = blockIdx.x * kBlock + threadIdx.x;
    float amax = 0.0f;
    bool work = s < ntris;
    uint32_t g = 0, inst = 0;
    if (work) { g = f2u(tris[s].v0.w); inst = shade[g].inst; }
    if (work && moved) { work = moved[inst] != 0u; tri_dirty[s] = work ? 1 : 0; }
    if (work) {
        const float* M = insts[inst].o2w;
        const F4 a = objtris[(size_t)g * 3], b = objtris[(size_t)g * 3 + 1], c = objtris[(size_t)g * 3 + 2];
        const f3 w0 = xform_point(M, mk3(a.x, a.y, a.z)), w1 = xform_point(M, mk3(b.x, b.y, b.z)), w2 = xform_point(M, mk3(c.x, c.y, c.z));
        const f3 e1 = w1 - w0, e2 = w2 - w0;
        const bool hide = VIS && hidden[inst] != 0u;
        tris[s].v0 = {w0.x, w0.y, w0.z, u2f(g)};
        tris[s].e1 = {e1.x, e1.y, e1.z, hide ? __builtin_inff() : tri_det_floor(e1, e2)};        // (as the host build: same operations, same bits; +inf: the never-hit record)
        tris[s].e2 = {e2.x, e2.y, e2.z, 0.0f};
        if (!hide) amax = fmaxf(fmaxf(fmaxf(fabsf(w0.x), fabsf(w0.y)), fmaxf(fabsf(w0.z), fabsf(w1.x))), fmaxf(fmaxf(fabsf(w1.y), fabsf(w1.z)), fmaxf(fmaxf(fabsf(w2.x), fabsf(w2.y)), fabsf(w2.z))));
    }
    atomicMax(&s_max, f2u(amax));                      // non-negative floats order like their bit patterns
    __syncthreads();
    if (threadIdx.x == 0 && s_max) atomicMax(scale_bits, s_max);
}

// Empty children: a leaf slot none of whose triangles is visible (e1.w == +inf), and an internal child whose subtree holds none (its float box in node_aabb is INVERTED,
// min = +inf > max = -inf, which is also what a clean child of the partial refit hands up), is left out of the node's box and quantised to near byte 255 / far byte 0 on every
// axis, an interval the slab test cannot enter.  imask and trivalid keep the topology, so showing the instance again is the same refit.  A node without visible content stores
// the inverted box and a fixed record (origin 0, unit grid, every child empty); the root may be such a node.
template <bool VIS>
__global__ __launch_bounds__(kBlock) void k_refit_nodes(Node8GPU* __restrict__ nodes, uint32_t first, uint32_t count, const TriGPU* __restrict__ tris,
                                                        F4* __restrict__ node_aabb /* 2 per node: min, max */, const uint32_t* __restrict__ scale_bits,
                                                        const uint8_t* __restrict__ tri_dirty, uint8_t* __restrict__ node_dirty) {
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t n = first + i;
    Node8GPU N = nodes[n];
    const float pad = 2e-6f * u2f(*scale_bits);          // the host build's bvh_pad (rtx_scene_host.cpp)
    const uint32_t imask = N.e_imask >> 24;
    if (tri_dirty) {                                      // partial refit: anything below this node touched?
        bool dirty = false;
        const uint32_t nint = (uint32_t)__builtin_popcount(imask);
        for (uint32_t k = 0; k < nint; k++) dirty = dirty || node_dirty[N.child_base + k] != 0;
        const uint32_t nleaf = (uint32_t)__builtin_popcount(N.trivalid);
        for (uint32_t k = 0; k < nleaf; k++) dirty = dirty || tri_dirty[N.tri_base + k] != 0;
        node_dirty[n] = dirty ? 1 : 0;
        if (!dirty) return;                               // node_aabb[n] and the quantised node stay what the last refit made them
    }
    float cmn[8][3], cmx[8][3];
    float bmn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, bmx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    uint32_t rank = 0, tri_at = N.tri_base, used = 0, empty = 0;
#pragma unroll
    for (int sl = 0; sl < 8; sl++) {
        const uint32_t nib = (N.trivalid >> (4 * sl)) & 0xfu;
        for (int a = 0; a < 3; a++) { cmn[sl][a] = 0.0f; cmx[sl][a] = 0.0f; }
        if ((imask >> sl) & 1u) {
            const F4 mn = node_aabb[2 * (size_t)(N.child_base + rank)], mx = node_aabb[2 * (size_t)(N.child_base + rank) + 1];
            rank++;
            if (VIS && mn.x > mx.x) { empty |= 1u << sl; continue; }   // nothing visible below this child
            cmn[sl][0] = mn.x; cmn[sl][1] = mn.y; cmn[sl][2] = mn.z; cmx[sl][0] = mx.x; cmx[sl][1] = mx.y; cmx[sl][2] = mx.z;
        } else if (nib) {
            float mn[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()}, mx[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
            const uint32_t cnt = (uint32_t)__builtin_popcount(nib);
            bool visible = false;
            for (uint32_t k = 0; k < cnt; k++, tri_at++) {
                const TriGPU T = tris[tri_at];
                if (VIS && T.e1.w == __builtin_inff()) continue;        // a hidden instance's triangle: in its slot, in no box
                visible = true;
                const float v[3][3] = {{T.v0.x, T.v0.y, T.v0.z}, {T.v0.x + T.e1.x, T.v0.y + T.e1.y, T.v0.z + T.e1.z}, {T.v0.x + T.e2.x, T.v0.y + T.e2.y, T.v0.z + T.e2.z}};
                for (int a = 0; a < 3; a++) { mn[a] = fminf(mn[a], fminf(v[0][a], fminf(v[1][a], v[2][a]))); mx[a] = fmaxf(mx[a], fmaxf(v[0][a], fmaxf(v[1][a], v[2][a]))); }
            }
            if (VIS && !visible) { empty |= 1u << sl; continue; }
            for (int a = 0; a < 3; a++) { cmn[sl][a] = mn[a] - pad; cmx[sl][a] = mx[a] + pad; }
        } else continue;
        used |= 1u << sl;
        for (int a = 0; a < 3; a++) { bmn[a] = fminf(bmn[a], cmn[sl][a]); bmx[a] = fmaxf(bmx[a], cmx[sl][a]); }
    }
    if (VIS) { node_aabb[2 * (size_t)n] = {bmn[0], bmn[1], bmn[2], 0.0f}; node_aabb[2 * (size_t)n + 1] = {bmx[0], bmx[1], bmx[2], 0.0f}; }      // (!used: inverted, a parent reads it as empty)
    if (!used) { for (int a = 0; a < 3; a++) { bmn[a] = 0.0f; bmx[a] = 0.0f; } }
    if (!VIS) { node_aabb[2 * (size_t)n] = {bmn[0], bmn[1], bmn[2], 0.0f}; node_aabb[2 * (size_t)n + 1] = {bmx[0], bmx[1], bmx[2], 0.0f}; }     // (a node without any child: a point, as ever)
    // byte grid: p = box minimum, smallest power of two with 255 steps covering the (upward-rounded) extent
    uint32_t eb[3]; float inv_step[3];
    for (int a = 0; a < 3; a++) {
        const float ext = sub_up(bmx[a], bmn[a]);
        int e = -120;
        if (ext > 0.0f) {
            int k; const float m = frexpf(ext, &k);            // ext = m * 2^k, m in [0.5, 1)
            e = m <= 0.99609375f ? k - 8 : k - 7;               // 255 * 2^(k-8) = 0.99609375 * 2^k
            if (e < -120) e = -120;
            if (e > 120) e = 120;                               // (cannot cover; such coordinates are rejected at commit)
        }
        if (VIS && !used) e = 0;
        eb[a] = (uint32_t)(e + 127); inv_step[a] = u2f((uint32_t)(127 - e) << 23);
    }
    N.px = bmn[0]; N.py = bmn[1]; N.pz = bmn[2];
    N.e_imask = eb[0] | eb[1] << 8 | eb[2] << 16 | imask << 24;
    for (int r = 0; r < 12; r++) N.q[r] = 0;
#pragma unroll
    for (int sl = 0; sl < 8; sl++) {
        if (VIS && ((empty >> sl) & 1u)) for (int a = 0; a < 3; a++) N.q[2 * a + (sl >> 2)] |= 255u << (8 * (sl & 3));      // near byte 255, far byte 0
        if (!((used >> sl) & 1u)) continue;
        for (int a = 0; a < 3; a++) {
            float qlo = floorf(sub_down(cmn[sl][a], bmn[a]) * inv_step[a]), qhi = ceilf(sub_up(cmx[sl][a], bmn[a]) * inv_step[a]);
            qlo = fminf(255.0f, fmaxf(0.0f, qlo)); qhi = fminf(255.0f, fmaxf(0.0f, qhi));
            N.q[2 * a + (sl >> 2)] |= (uint32_t)qlo << (8 * (sl & 3));
            N.q[2 * (3 + a) + (sl >> 2)] |= (uint32_t)qhi << (8 * (sl & 3));
        }
    }
    nodes[n] = N;
}

// Tree quality after refits: the sum over the wide nodes of the half-area of their float box (node_aabb, as the last refit left it).  Divided by the root's half-area that is
// the expected number of node visits of a random line through the scene — what work_per_ray.node_steps tracks —, so a refitted tree whose boxes have grown to cover their
// object shows it here.  The value steers a rebuild decision (RTX_OPT_DEFORM_REBUILD), so two runs must give the same bits: a wave reduction in a fixed order, the four wave
// sums of a workgroup added in wave order, ONE partial per workgroup (a plain store; the host adds them in index order, in double) — no float atomics.  partial[gridDim.x] =
// the root's half-area.  A workgroup reads node_aabb only: it does not depend on another workgroup of the launch.
__device__ __forceinline__ float box_half_area(const F4 mn, const F4 mx) {
    if (mn.x > mx.x) return 0.0f;                          // a node without visible content (k_refit_nodes): nothing to visit
    const float ex = mx.x - mn.x, ey = mx.y - mn.y, ez = mx.z - mn.z;
    return ex * ey + ey * ez + ez * ex;
}
__global__ __launch_bounds__(kBlock) void k_tree_cost(const F4* __restrict__ node_aabb, uint32_t nnodes, float* __restrict__ partial) {
    __shared__ float s_wave[kBlock / 64];
    const uint32_t n = blockIdx.x * kBlock + threadIdx.x;
    float a = n < nnodes ? box_half_area(node_aabb[2 * (size_t)n], node_aabb[2 * (size_t)n + 1]) : 0.0f;
    if (n == 0) partial[gridDim.x] = a;
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63u) == 0) s_wave[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) { float t = s_wave[0]; for (int w = 1; w < kBlock / 64; w++) t += s_wave[w]; partial[blockIdx.x] = t; }
}

void launch_refit(hipStream_t st, Node8GPU* nodes, const uint32_t* level_start, uint32_t nlevels, TriGPU* tris, uint32_t ntris, const TriShade* shade,
                  const InstGPU* insts, const F4* objtris, F4* node_aabb, uint32_t* scale_bits, const uint32_t* moved, uint8_t* tri_dirty, uint8_t* node_dirty, const uint32_t* hidden) {
    if (!moved) tri_dirty = nullptr;                              // full refit
    auto refit_tris = hidden ? k_refit_tris<true> : k_refit_tris<false>;
    auto refit_nodes = hidden ? k_refit_nodes<true> : k_refit_nodes<false>;
    if (ntris) hipLaunchKernelGGL(refit_tris, dim3((ntris + kBlock - 1) / kBlock), dim3(kBlock), 0, st, tris, ntris, shade, insts, objtris, scale_bits, moved, tri_dirty, hidden);
    for (uint32_t l = nlevels; l-- > 0;) {                       // deepest level first: children are refitted before their parents
        const uint32_t first = level_start[l], count = level_start[l + 1] - first;
        if (count) hipLaunchKernelGGL(refit_nodes, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, st, nodes, first, count, tris, node_aabb, scale_bits, (const uint8_t*)tri_dirty, node_dirty);
    }
}
uint32_t tree_cost_partials(uint32_t nnodes) { return (nnodes + kBlock - 1) / kBlock + 1u; }
void launch_tree_cost(hipStream_t st, const F4* node_aabb, uint32_t nnodes, float* partial) {
    if (nnodes) hipLaunchKernelGGL(k_tree_cost, dim3((nnodes + kBlock - 1) / kBlock), dim3(kBlock), 0, st, node_aabb, nnodes, partial);
}

}  // namespace rtx

// rtx_bvh_build.cpp — the host's binary BVH builder: options, refit, the top-down binned-SAH builder with spatial splits and re-insertion, the PLOC host twin of
// the GPU build and the top of its tree.  No HIP calls in this file.
#include "rtx_bvh_host.hpp"
#include "rtx_wide.hpp"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <system_error>
#include <thread>

namespace rtx {

// ------------------------------------------------------------------------------------------------
// binned SAH BVH2 (16 bins, leaves of <= 4 triangles unless a split is impossible, hard cap 8)
// ------------------------------------------------------------------------------------------------
BvhBuildOptions& bvh_build_options() {
    static BvhBuildOptions o;
    static bool env_read = false;
    if (!env_read) {                                       // tooling: RTX_BVH="reinsert=2,split=1e-5" (A/B runs of one binary)
        env_read = true;
        if (const char* e = getenv("RTX_BVH")) {
            std::string s = e; size_t at = 0;
            while (at < s.size()) {
                size_t end = s.find(',', at); if (end == std::string::npos) end = s.size();
                const std::string kv = s.substr(at, end - at); const size_t eq = kv.find('=');
                if (eq != std::string::npos && !bvh_build_option(o, kv.substr(0, eq).c_str(), atof(kv.c_str() + eq + 1))) fprintf(stderr, "[rtx] RTX_BVH: unknown key in '%s'\n", kv.c_str());
                at = end + 1;
            }
        }
    }
    return o;
}
bool bvh_build_option(const char* key, double v) { return bvh_build_option(bvh_build_options(), key, v); }
bool bvh_build_option(BvhBuildOptions& o, const char* key, double v) {
    const std::string k = key ? key : "";
    if (k == "bins") o.bins = (int)v;
    else if (k == "sweep") o.sweep_below = (uint32_t)v;
    else if (k == "tri_cost") o.tri_cost = v;
    else if (k == "threads") o.threads = (int)v;
    else if (k == "ploc") o.ploc_radius = (int)v;
    else if (k == "ploc_top") o.ploc_top = (uint32_t)v;
    else if (k == "leaf_stop") o.leaf_stop = (uint32_t)v;
    else if (k == "split") o.split_alpha = v;
    else if (k == "slot_assign") o.slot_assign = (int)v;
    else if (k == "split_budget") o.split_budget = v;
    else if (k == "reinsert") o.reinsert_passes = (int)v;
    else if (k == "reinsert_frac") o.reinsert_frac = v;
    else if (k == "reinsert_cap") o.reinsert_cap = (uint32_t)v;
    else return false;
    return true;
}

// Refit: keep the topology (node links, leaf order), recompute every child box bottom-up.  Nodes are stored
// breadth-first, so a child always has a larger index than its parent: one reverse sweep suffices.
void refit_bvh(const std::vector<float>& wtri, float pad_abs, std::vector<NodeGPU>& nodes, const std::vector<uint32_t>& order) {
    auto child_box = [&](int32_t child, float* mn, float* mx) {
        for (int a = 0; a < 3; a++) { mn[a] = INFINITY; mx[a] = -INFINITY; }
        if (child == kEmptyChild) return;
        if (child < 0) {                                  // leaf: bounds of its triangles
            const uint32_t v = ~(uint32_t)child, first = v >> 3, cnt = (v & 7u) + 1u;
            for (uint32_t k = 0; k < cnt; k++) {
                const float* t = &wtri[(size_t)order[first + k] * 9];
                for (int vtx = 0; vtx < 3; vtx++) for (int a = 0; a < 3; a++) { mn[a] = std::min(mn[a], t[vtx * 3 + a]); mx[a] = std::max(mx[a], t[vtx * 3 + a]); }
            }
            for (int a = 0; a < 3; a++) { mn[a] -= pad_abs; mx[a] += pad_abs; }
        } else {                                          // internal: union of its two (already refitted, already padded) child boxes
            const NodeGPU& N = nodes[child];
            const float amn[3] = {N.a.x, N.a.y, N.a.z}, amx[3] = {N.a.w, N.b.x, N.b.y}, bmn[3] = {N.b.z, N.b.w, N.c.x}, bmx[3] = {N.c.y, N.c.z, N.c.w};
            for (int a = 0; a < 3; a++) { mn[a] = std::min(amn[a], bmn[a]); mx[a] = std::max(amx[a], bmx[a]); }
        }
    };
    for (size_t i = nodes.size(); i-- > 0;) {
        NodeGPU& N = nodes[i];
        float mn[3], mx[3];
        child_box((int32_t)f2u(N.d.x), mn, mx);
        N.a = {mn[0], mn[1], mn[2], mx[0]}; N.b.x = mx[1]; N.b.y = mx[2];
        child_box((int32_t)f2u(N.d.y), mn, mx);
        N.b.z = mn[0]; N.b.w = mn[1]; N.c = {mn[2], mx[0], mx[1], mx[2]};
    }
}

namespace {
struct Box { float mn[3], mx[3]; };
inline Box empty_box() { Box b; for (int a = 0; a < 3; a++) { b.mn[a] = INFINITY; b.mx[a] = -INFINITY; } return b; }
inline void grow(Box& b, const Box& o) { for (int a = 0; a < 3; a++) { b.mn[a] = std::min(b.mn[a], o.mn[a]); b.mx[a] = std::max(b.mx[a], o.mx[a]); } }
inline float half_area(const Box& b) {
    float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    if (dx < 0) return 0.0f;
    return dx * dy + dy * dz + dz * dx;
}
struct TmpNode { Box box; int32_t left = -1, right = -1; uint32_t first = 0, count = 0; };

// ---- the top-down builder works on REFERENCES (box, triangle): a spatial split (Stich, Friedrich, Dietrich, "Spatial Splits in Bounding Volume
//      Hierarchies", HPG 2009) may hand a triangle to both sides of a plane, each side keeping the box of ITS part.  The closest hit is defined as
//      the minimum over all triangles (ties: lowest id) and any hit as existence, so a triangle referenced from two leaves changes no result; what
//      has to hold is COVERAGE: every point of a triangle lies in the box of one of its references and in every box above it.  Parts are clipped
//      in double and their boxes rounded outward, so the pieces' boxes cover the triangle like the whole box did. ----
struct Ref { Box box; uint32_t tri; };
inline float f_below(float x) { return std::nextafterf(x, -INFINITY); }
inline float f_above(float x) { return std::nextafterf(x, INFINITY); }
inline Box intersect(const Box& a, const Box& b) { Box r; for (int k = 0; k < 3; k++) { r.mn[k] = std::max(a.mn[k], b.mn[k]); r.mx[k] = std::min(a.mx[k], b.mx[k]); } return r; }
// parts of triangle t9 inside `in` on either side of the plane x[axis] = pos
inline void split_ref(const float* t9, const Box& in, int axis, float pos, Box& L, Box& R) {
    L = empty_box(); R = empty_box();
    auto add = [](Box& b, const double* p, bool exact) {
        for (int k = 0; k < 3; k++) {
            const float f = (float)p[k];
            const float lo = exact ? f : ((double)f > p[k] ? f_below(f) : f), hi = exact ? f : ((double)f < p[k] ? f_above(f) : f);
            b.mn[k] = std::min(b.mn[k], exact ? f : f_below(lo)); b.mx[k] = std::max(b.mx[k], exact ? f : f_above(hi));
        }
    };
    for (int e = 0; e < 3; e++) {
        const float* a = t9 + 3 * e; const float* b = t9 + 3 * ((e + 1) % 3);
        const double pa[3] = {a[0], a[1], a[2]};
        if (a[axis] <= pos) add(L, pa, true);
        if (a[axis] >= pos) add(R, pa, true);
        if ((a[axis] < pos && b[axis] > pos) || (a[axis] > pos && b[axis] < pos)) {
            const double t = std::min(1.0, std::max(0.0, ((double)pos - (double)a[axis]) / ((double)b[axis] - (double)a[axis])));
            double p[3]; for (int k = 0; k < 3; k++) p[k] = (double)a[k] + t * ((double)b[k] - (double)a[k]);
            p[axis] = pos;
            add(L, p, false); add(R, p, false);
        }
    }
    L.mx[axis] = std::min(L.mx[axis], pos); R.mn[axis] = std::max(R.mn[axis], pos);
    L = intersect(L, in); R = intersect(R, in);
    L.mx[axis] = std::max(L.mx[axis], L.mn[axis]); R.mx[axis] = std::max(R.mx[axis], R.mn[axis]);    // (a sliver part keeps a valid, zero-width box)
}
inline bool valid_box(const Box& b) { return b.mn[0] <= b.mx[0] && b.mn[1] <= b.mx[1] && b.mn[2] <= b.mx[2]; }

// Insertion-based optimisation of the binary tree (Bittner, Hapala, Havran, "Fast Insertion-Based Optimization of Bounding Volume Hierarchies", CGF 2013; the
// per-node search of Meister & Bittner, "Parallel Reinsertion for Bounding Volume Hierarchy Optimization", EG 2018): a subtree is cut out and put back where it
// enlarges the fewest / smallest boxes (branch-and-bound over the induced surface-area cost).  Topology only: leaves and their references stay as they are.
void reinsert_pass(std::vector<TmpNode>& tn, std::vector<int32_t>& parent, double frac) {
    const size_t n = tn.size();
    // the candidates: largest boxes first, ties in index order (what a stable sort by area gives) — but only the first `frac` of that order is wanted, so: select, then sort
    // the selection (a full stable_sort of 1.9 M nodes with the area recomputed in every comparison was 2/3 of the pass's time on the street scene)
    std::vector<std::pair<float, uint32_t>> keyed; keyed.reserve(n);
    for (size_t i = 1; i < n; i++) if (parent[i] > 0) keyed.push_back({half_area(tn[i].box), (uint32_t)i});      // not the root, not a child of the root (the root stays node 0)
    const auto before = [](const std::pair<float, uint32_t>& a, const std::pair<float, uint32_t>& b) { return a.first > b.first || (a.first == b.first && a.second < b.second); };
    const size_t keep = (size_t)((double)keyed.size() * frac);
    if (keep < keyed.size()) std::nth_element(keyed.begin(), keyed.begin() + keep, keyed.end(), before);
    std::sort(keyed.begin(), keyed.begin() + keep, before);
    std::vector<uint32_t> cand(keep);
    for (size_t i = 0; i < keep; i++) cand[i] = keyed[i].second;
    auto refit_up = [&](int32_t a) {
        for (; a >= 0; a = parent[a]) {
            Box b = tn[tn[a].left].box; grow(b, tn[tn[a].right].box);
            if (!memcmp(&b, &tn[a].box, sizeof(Box))) break;
            tn[a].box = b;
        }
    };
    struct It { float bound; float induced; int32_t node; };
    auto cmp = [](const It& a, const It& b) { return a.bound > b.bound; };
    std::vector<It> pq;
    for (uint32_t x : cand) {
        const int32_t p = parent[x];
        if (p <= 0) continue;                                   // (moves may have lifted x to the root's children)
        const int32_t g = parent[p], s = tn[p].left == (int32_t)x ? tn[p].right : tn[p].left;
        // cut x (and its parent node p) out
        (tn[g].left == p ? tn[g].left : tn[g].right) = s; parent[s] = g;
        refit_up(g);
        const Box xb = tn[x].box; const float xa = half_area(xb);
        float best = INFINITY; int32_t best_node = s;
        pq.clear();
        pq.push_back({0.0f, 0.0f, tn[0].left}); pq.push_back({0.0f, 0.0f, tn[0].right});
        {   // the root's own enlargement is paid by every position alike: leave it out
        }
        std::make_heap(pq.begin(), pq.end(), cmp);
        while (!pq.empty()) {
            std::pop_heap(pq.begin(), pq.end(), cmp); const It it = pq.back(); pq.pop_back();
            if (it.bound + xa >= best) break;
            Box u = tn[it.node].box; grow(u, xb);
            const float direct = half_area(u), total = it.induced + direct;
            if (total < best) { best = total; best_node = it.node; }
            if (!tn[it.node].count) {
                const float ind = it.induced + direct - half_area(tn[it.node].box);
                if (ind + xa < best) {
                    pq.push_back({ind, ind, tn[it.node].left}); std::push_heap(pq.begin(), pq.end(), cmp);
                    pq.push_back({ind, ind, tn[it.node].right}); std::push_heap(pq.begin(), pq.end(), cmp);
                }
            }
        }
        // put it back: p becomes the parent of (best_node, x) where best_node was
        const int32_t gb = parent[best_node];
        (tn[gb].left == best_node ? tn[gb].left : tn[gb].right) = p; parent[p] = gb;
        tn[p].left = best_node; tn[p].right = (int32_t)x; parent[best_node] = p; parent[x] = p;
        tn[p].box = tn[best_node].box; grow(tn[p].box, xb);
        refit_up(gb);
    }
}
// ---- PLOC: parallel locally-ordered clustering (Meister & Bittner, "Parallel Locally-Ordered Clustering for Bounding Volume Hierarchy Construction", TVCG 2018) — the
//      BOTTOM-UP builder of the GPU build (csrc/rtx_build.hip: RTX_OPT_GPU_BUILD), restated here so that its trees can be judged by work per ray without a GPU
//      (tools/bvh_lab: ploc=<radius>) and so that the device code has a host twin to be compared with node for node.  Triangles are sorted along the Morton curve of
//      their box centres (63 bits, ties by triangle id); every cluster looks `radius` places to either side for the neighbour whose union with it has the smallest
//      surface area; mutual nearest neighbours merge; repeat until one cluster is left.  Everything is a pure function of the input order, so host and device agree. ----
struct PlocNode { Box box; int32_t left, right; uint32_t tri; };
// clusters until at most `stop_at` are left; pool: [0, n) leaves in Morton order, internal nodes appended in creation order (iteration by iteration, left partners in cluster order)
void ploc_clusters(const std::vector<Ref>& refs, const Box& scene, int radius, uint32_t stop_at, std::vector<PlocNode>& pn, std::vector<int32_t>& cl) {
    const uint32_t n = (uint32_t)refs.size();
    // Morton keys of the box centres on a 2^21 grid over the scene's box (float arithmetic, the device's formula: rtx_wide.hpp ploc_morton)
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    float lo[3], inv[3];
    ploc_grid(scene.mn, scene.mx, lo, inv);
    auto wb = [](const Box& b) { WBox w; for (int a = 0; a < 3; a++) { w.mn[a] = b.mn[a]; w.mx[a] = b.mx[a]; } return w; };
    for (uint32_t i = 0; i < n; i++) keyed[i] = {ploc_morton(wb(refs[i].box), lo, inv), i};
    std::sort(keyed.begin(), keyed.end());
    pn.clear(); pn.reserve((size_t)2 * n);
    for (uint32_t i = 0; i < n; i++) { const Ref& r = refs[keyed[i].second]; pn.push_back(PlocNode{r.box, -1, -1, r.tri}); }
    cl.resize(n); for (uint32_t i = 0; i < n; i++) cl[i] = (int32_t)i;
    std::vector<int32_t> nn, nxt;
    while (cl.size() > std::max<size_t>(1, stop_at)) {
        const int m = (int)cl.size();
        nn.assign(m, -1);
        for (int i = 0; i < m; i++) nn[i] = ploc_nearest(i, m, radius, [&](int j) { return wb(pn[cl[j]].box); });      // nearest neighbour within the window (rtx_wide.hpp)
        nxt.clear();
        for (int i = 0; i < m; i++) {
            const int j = nn[i];
            if (j >= 0 && nn[j] == i) {                       // mutual: the lower position becomes the new node, the higher one disappears
                if (i < j) { PlocNode N; N.box = pn[cl[i]].box; grow(N.box, pn[cl[j]].box); N.left = cl[i]; N.right = cl[j]; N.tri = 0; pn.push_back(N); nxt.push_back((int32_t)pn.size() - 1); }
            } else nxt.push_back(cl[i]);
        }
        cl.swap(nxt);
    }
}
// hang the PLOC subtree `src` of the pool below node `dst` of the build's tree (leaves of ONE triangle each, depth-first left to right)
void ploc_expand(const std::vector<PlocNode>& pn, int32_t src0, int32_t dst0, uint32_t depth0, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth) {
    struct It { int32_t src, dst; uint32_t depth; };
    std::vector<It> st; st.push_back({src0, dst0, depth0});
    while (!st.empty()) {
        const It it = st.back(); st.pop_back();
        max_depth = std::max(max_depth, it.depth);
        const PlocNode& N = pn[it.src];
        tn[it.dst].box = N.box;
        if (N.left < 0) { tn[it.dst].first = (uint32_t)order.size(); tn[it.dst].count = 1; tn[it.dst].left = tn[it.dst].right = -1; order.push_back(N.tri); continue; }
        const int32_t l = (int32_t)tn.size(); tn.emplace_back(); const int32_t r = (int32_t)tn.size(); tn.emplace_back();
        tn[it.dst].left = l; tn[it.dst].right = r; tn[it.dst].count = 0;
        st.push_back({N.right, r, it.depth + 1}); st.push_back({N.left, l, it.depth + 1});
    }
}
struct Job { int32_t node; uint32_t count, depth; };
constexpr int NB = 16, NS = 16;
inline float cen(const Ref& r, int a) { return 0.5f * (r.box.mn[a] + r.box.mx[a]); }
// PARALLEL top-down phase (round 4: 9.3 of the 10 s a commit of the 3.8 M-triangle street took were this function, on one core).  The serial loop runs until a node has at
// most `cutoff` references, moves that node's references out as a TASK and goes on; the tasks then run the same loop on private stacks in a thread pool, and their
// subtrees are spliced back in the order in which they were cut.  A subtree is a function of its references alone (no spatial-split budget is shared: with spatial
// splits the build stays serial), `cutoff` depends on the triangle count only, and the nodes are renumbered into the serial loop's creation order afterwards — so the tree
// is THE SAME tree, node for node, as the serial build's, whatever the number of threads.
struct Task { int32_t node; uint32_t depth; std::vector<Ref> refs; std::vector<TmpNode> tn; std::vector<uint32_t> order; uint32_t max_depth = 0; };

// The top-down loop.  What one build fixes for all its runs is the struct; a run works on the state it is handed: the reference stack `refs` (all of it: the references
// of the subtree to build, root at depth `depth0`), the tree `tn` and the leaf order `order` it appends to (the subtree's root becomes the next node of tn), the depth
// and reference counters it updates.  may_defer: subtrees of at most `cutoff` references are cut out into `tasks` instead of being built.
struct TopDown {
    const BvhBuildOptions& opt; const float* wtri; const bool spatial; const float spatial_min; const size_t ref_budget; const uint32_t cutoff;
    std::vector<Task>& tasks;
    void operator()(std::vector<Ref>& refs, uint32_t depth0, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth, size_t& refs_total, bool may_defer) const;
};
void TopDown::operator()(std::vector<Ref>& refs, uint32_t depth0, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth, size_t& refs_total, bool may_defer) const {
    std::vector<Job> st; tn.emplace_back(); st.push_back({0, (uint32_t)refs.size(), depth0});
    std::vector<uint32_t> sweep_ids; std::vector<float> sweep_ra; std::vector<Ref> tmp;
    while (!st.empty()) {
        const Job j = st.back(); st.pop_back();
        max_depth = std::max(max_depth, j.depth);
        Ref* R = refs.data() + (refs.size() - j.count);                              // this node's references: the top of the reference stack
        if (may_defer && j.count <= cutoff && j.count > 4u) {                         // cut this subtree out: a task of the pool
            tasks.emplace_back(); Task& T = tasks.back();
            T.node = j.node; T.depth = j.depth; T.refs.assign(R, R + j.count);
            refs.resize(refs.size() - j.count);
            continue;
        }
        Box nb = empty_box(), cb = empty_box();
        for (uint32_t i = 0; i < j.count; i++) {
            grow(nb, R[i].box);
            for (int a = 0; a < 3; a++) { const float c = cen(R[i], a); cb.mn[a] = std::min(cb.mn[a], c); cb.mx[a] = std::max(cb.mx[a], c); }
        }
        tn[j.node].box = nb;
        auto make_leaf = [&]() {
            tn[j.node].first = (uint32_t)order.size(); tn[j.node].count = j.count;
            for (uint32_t i = 0; i < j.count; i++) order.push_back(R[i].tri);
            refs.resize(refs.size() - j.count);
        };
        if (j.count <= opt.leaf_stop || j.depth >= 96u) {
            if (j.count <= 4) { make_leaf(); continue; }
        }
        // ---- best object split over 3 axes: full sweep over the sorted centroids for small nodes, bins above ----
        float best_cost = INFINITY, sweep_split = 0.0f; int best_axis = -1, best_bin = -1;
        Box best_lb = empty_box(), best_rb = empty_box();
        const bool sweep = j.count <= opt.sweep_below;
        if (sweep) {
            sweep_ids.resize(j.count); sweep_ra.resize(j.count);
            for (int a = 0; a < 3; a++) {
                if (!(cb.mx[a] - cb.mn[a] > 0.0f)) continue;
                for (uint32_t i = 0; i < j.count; i++) sweep_ids[i] = i;
                std::stable_sort(sweep_ids.begin(), sweep_ids.end(), [&](uint32_t x, uint32_t y) { return cen(R[x], a) < cen(R[y], a); });
                Box acc = empty_box();
                for (uint32_t i = j.count; i-- > 1;) { grow(acc, R[sweep_ids[i]].box); sweep_ra[i] = half_area(acc); }
                acc = empty_box();
                for (uint32_t i = 0; i + 1 < j.count; i++) {
                    grow(acc, R[sweep_ids[i]].box);
                    const float c0 = cen(R[sweep_ids[i]], a), c1 = cen(R[sweep_ids[i + 1]], a);
                    if (c0 == c1) continue;                                          // equal centroids stay together (the partition is by value)
                    const float cost = half_area(acc) * (float)(i + 1) + sweep_ra[i + 1] * (float)(j.count - i - 1);
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = (int)i; sweep_split = 0.5f * (c0 + c1); if (!(sweep_split > c0)) sweep_split = c1; }
                }
            }
        } else {
            for (int a = 0; a < 3; a++) {
                const float lo = cb.mn[a], ext = cb.mx[a] - cb.mn[a];
                if (!(ext > 0.0f)) continue;
                Box bb[NB]; uint32_t bc[NB];
                for (int b = 0; b < NB; b++) { bb[b] = empty_box(); bc[b] = 0; }
                const float k = (float)NB / ext;
                for (uint32_t i = 0; i < j.count; i++) {
                    int b = (int)((cen(R[i], a) - lo) * k); if (b >= NB) b = NB - 1; if (b < 0) b = 0;
                    grow(bb[b], R[i].box); bc[b]++;
                }
                float ra[NB]; uint32_t rc[NB]; Box rbx[NB]; Box acc = empty_box(); uint32_t c = 0;
                for (int b = NB - 1; b > 0; b--) { grow(acc, bb[b]); c += bc[b]; ra[b] = half_area(acc); rc[b] = c; rbx[b] = acc; }
                acc = empty_box(); c = 0;
                for (int b = 0; b < NB - 1; b++) {
                    grow(acc, bb[b]); c += bc[b];
                    if (!c || !rc[b + 1]) continue;
                    const float cost = half_area(acc) * (float)c + ra[b + 1] * (float)rc[b + 1];
                    if (cost < best_cost) { best_cost = cost; best_axis = a; best_bin = b; best_lb = acc; best_rb = rbx[b + 1]; }
                }
            }
        }
        const float leaf_cost = half_area(nb) * (float)j.count;
        // ---- spatial split candidate: only where the object split leaves the two sides overlapping (Stich et al., section 4.5) ----
        float sp_cost = INFINITY, sp_pos = 0.0f; int sp_axis = -1;
        if (spatial && j.count > 2 && refs_total < ref_budget) {
            bool try_it = best_axis < 0;
            if (!try_it) {
                if (sweep) {                                                         // (the sweep kept no boxes: rebuild the two sides of its best split)
                    best_lb = empty_box(); best_rb = empty_box();
                    for (uint32_t i = 0; i < j.count; i++) grow(cen(R[i], best_axis) < sweep_split ? best_lb : best_rb, R[i].box);
                }
                const Box ov = intersect(best_lb, best_rb);
                try_it = valid_box(ov) && half_area(ov) > spatial_min;
            }
            if (try_it) {
                for (int a = 0; a < 3; a++) {
                    const float lo = nb.mn[a], ext = nb.mx[a] - nb.mn[a];
                    if (!(ext > 0.0f)) continue;
                    Box bb[NS]; uint32_t enter[NS], leave[NS];
                    for (int b = 0; b < NS; b++) { bb[b] = empty_box(); enter[b] = leave[b] = 0; }
                    const float k = (float)NS / ext;
                    auto plane = [&](int b) { return lo + ext * ((float)b / (float)NS); };
                    for (uint32_t i = 0; i < j.count; i++) {
                        int b0 = (int)((R[i].box.mn[a] - lo) * k), b1 = (int)((R[i].box.mx[a] - lo) * k);
                        b0 = std::min(NS - 1, std::max(0, b0)); b1 = std::min(NS - 1, std::max(b0, b1));
                        while (b0 < b1 && plane(b0 + 1) <= R[i].box.mn[a]) b0++;               // (float binning vs. the plane positions used for chopping)
                        while (b1 > b0 && plane(b1) >= R[i].box.mx[a]) b1--;
                        enter[b0]++; leave[b1]++;
                        Box cur = R[i].box;
                        for (int b = b0; b < b1; b++) {
                            Box l, r; split_ref(&wtri[(size_t)R[i].tri * 9], cur, a, plane(b + 1), l, r);
                            if (valid_box(l)) grow(bb[b], l);
                            cur = r;
                            if (!valid_box(cur)) break;
                        }
                        if (valid_box(cur)) grow(bb[b1], cur);
                    }
                    float ra[NS]; uint32_t rc[NS]; Box acc = empty_box(); uint32_t c = 0;
                    for (int b = NS - 1; b > 0; b--) { grow(acc, bb[b]); c += leave[b]; ra[b] = half_area(acc); rc[b] = c; }
                    acc = empty_box(); c = 0;
                    for (int b = 0; b < NS - 1; b++) {
                        grow(acc, bb[b]); c += enter[b];
                        if (!c || !rc[b + 1] || c >= j.count || rc[b + 1] >= j.count) continue;       // a split that sends every reference to one side makes no progress
                        const float cost = half_area(acc) * (float)c + ra[b + 1] * (float)rc[b + 1];
                        if (cost < sp_cost) { sp_cost = cost; sp_axis = a; sp_pos = plane(b + 1); }
                    }
                }
            }
        }
        uint32_t nl = 0, nr = 0;                                                     // sizes of the two sides, laid out as [.. | left | right] on the reference stack
        bool split = false;
        if (sp_axis >= 0 && sp_cost < best_cost && (j.count > 4 || sp_cost + half_area(nb) < leaf_cost)) {
            // ---- spatial split with reference unsplitting (section 4.4): a straddling reference goes to both sides, or whole to one if that is cheaper ----
            tmp.clear();
            Box lb = empty_box(), rb = empty_box();
            std::vector<Ref> left, right, both;
            for (uint32_t i = 0; i < j.count; i++) {
                if (R[i].box.mx[sp_axis] <= sp_pos) { left.push_back(R[i]); grow(lb, R[i].box); }
                else if (R[i].box.mn[sp_axis] >= sp_pos) { right.push_back(R[i]); grow(rb, R[i].box); }
                else both.push_back(R[i]);
            }
            uint32_t cl = (uint32_t)(left.size() + both.size()), cr = (uint32_t)(right.size() + both.size());
            for (const Ref& r : both) {
                Box l, rr; split_ref(&wtri[(size_t)r.tri * 9], r.box, sp_axis, sp_pos, l, rr);
                const bool lv = valid_box(l), rv = valid_box(rr);
                Box lbs = lb, rbs = rb, lbw = lb, rbw = rb;
                if (lv) grow(lbs, l); if (rv) grow(rbs, rr); grow(lbw, r.box); grow(rbw, r.box);
                const float c_split = half_area(lbs) * (float)cl + half_area(rbs) * (float)cr;
                const float c_left = half_area(lbw) * (float)cl + half_area(rb) * (float)(cr - 1);
                const float c_right = half_area(lb) * (float)(cl - 1) + half_area(rbw) * (float)cr;
                if (lv && rv && c_split <= c_left && c_split <= c_right && refs_total < ref_budget) {
                    left.push_back({l, r.tri}); right.push_back({rr, r.tri}); lb = lbs; rb = rbs; refs_total++;
                } else if ((c_left <= c_right && cr > 1) || !rv || cl <= 1) { left.push_back(r); lb = lbw; cr--; }
                else { right.push_back(r); rb = rbw; cl--; }
            }
            nl = (uint32_t)left.size(); nr = (uint32_t)right.size();
            if (nl && nr && nl < j.count + both.size() && nr < j.count + both.size() && !(nl >= j.count && nr >= j.count)) {
                refs.resize(refs.size() - j.count);
                refs.insert(refs.end(), left.begin(), left.end()); refs.insert(refs.end(), right.begin(), right.end());
                split = true;
            } else { refs_total -= (nl + nr > j.count) ? (nl + nr - j.count) : 0; nl = nr = 0; }
        }
        if (!split && best_axis >= 0 && (j.count > 4 || best_cost + half_area(nb) * 1.0f < leaf_cost)) {
            const float lo = cb.mn[best_axis], k = (float)NB / (cb.mx[best_axis] - cb.mn[best_axis]);
            Ref* mid = sweep ? std::stable_partition(R, R + j.count, [&](const Ref& r) { return cen(r, best_axis) < sweep_split; })
                             : std::stable_partition(R, R + j.count, [&](const Ref& r) { int b = (int)((cen(r, best_axis) - lo) * k); if (b >= NB) b = NB - 1; if (b < 0) b = 0; return b <= best_bin; });
            nl = (uint32_t)(mid - R); nr = j.count - nl;
            split = nl > 0 && nr > 0;
        }
        if (!split) {
            if (j.count <= 4) { make_leaf(); continue; }            // leaves hold at most 4 triangles (the wide node's 4-bit slots)
            nl = j.count / 2; nr = j.count - nl;                    // degenerate (all centroids equal) or forced: median split by index
        }
        const int32_t l = (int32_t)tn.size(); tn.emplace_back();
        const int32_t r = (int32_t)tn.size(); tn.emplace_back();
        tn[j.node].left = l; tn[j.node].right = r;
        st.push_back({l, nl, j.depth + 1});
        st.push_back({r, nr, j.depth + 1});                          // the right side lies on top of the reference stack: it is processed first
    }
}
}  // namespace

// the tasks the serial part cut out, on up to `threads` threads (0: up to 16 of the machine's) and this one
static void run_tasks(const TopDown& top_down, std::vector<Task>& tasks, int threads) {
    std::atomic<size_t> next{0};
    auto work = [&]() {
        for (size_t k = next.fetch_add(1); k < tasks.size(); k = next.fetch_add(1)) {
            Task& T = tasks[k];
            size_t local_total = 0;
            T.tn.reserve(2 * T.refs.size() + 2); T.order.reserve(T.refs.size());
            top_down(T.refs, T.depth, T.tn, T.order, T.max_depth, local_total, false);
        }
    };
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nthreads = std::min<size_t>(tasks.size(), threads > 1 ? (unsigned)threads : std::min<unsigned>(hw ? hw : 4u, 16u));
    std::vector<std::thread> pool;
    for (size_t t = 1; t < nthreads; t++) { try { pool.emplace_back(work); } catch (const std::system_error&) { break; } }      // (no more threads to be had: the ones that started and this one do the work)
    work();
    for (std::thread& t : pool) t.join();
}
// the tasks' subtrees back into the tree, in the order in which they were cut, and the nodes renumbered into the serial loop's creation order
static void splice_tasks(std::vector<Task>& tasks, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth) {
    for (Task& T : tasks) {                                          // splice: local node 0 is the node the task was cut at, local i > 0 becomes base + i - 1
        const int32_t base = (int32_t)tn.size(); const uint32_t obase = (uint32_t)order.size();
        auto gid = [&](int32_t i) { return i == 0 ? T.node : base + i - 1; };
        for (size_t i = 0; i < T.tn.size(); i++) {
            TmpNode n = T.tn[i];
            if (n.count) n.first += obase; else { n.left = gid(n.left); n.right = gid(n.right); }
            if (i == 0) tn[T.node] = n; else tn.push_back(n);
        }
        order.insert(order.end(), T.order.begin(), T.order.end());
        max_depth = std::max(max_depth, T.max_depth);
    }
    // the serial loop's node numbering: a node's two children are created when it is processed, and the right child is processed first
    std::vector<int32_t> new_id(tn.size(), -1), stack_; int32_t nid = 1; new_id[0] = 0; stack_.push_back(0);
    while (!stack_.empty()) {
        const int32_t x = stack_.back(); stack_.pop_back();
        if (tn[x].count) continue;
        new_id[tn[x].left] = nid++; new_id[tn[x].right] = nid++;
        stack_.push_back(tn[x].left); stack_.push_back(tn[x].right);
    }
    std::vector<TmpNode> ren(tn.size());
    for (size_t i = 0; i < tn.size(); i++) { TmpNode n = tn[i]; if (!n.count) { n.left = new_id[n.left]; n.right = new_id[n.right]; } ren[new_id[i]] = n; }
    tn.swap(ren);
}

// the top-down builder (+ the re-insertion passes) over a set of references: fills the temporary tree `tn` (root = node 0; leaves hold [first, first + count) of `order`)
static void build_tmp_tree(std::vector<Ref>& refs, const Box& scene, const BvhBuildOptions& opt, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth,
                           BuildStopwatch& sw, const float* wtri /* 9 floats per triangle: spatial splits clip against them (nullptr: no splits) */) {
    const uint32_t nt = (uint32_t)refs.size();
    order.clear(); order.reserve(nt);
    tn.clear(); tn.reserve((size_t)2 * nt + 2);
    max_depth = 0;
    // spatial splits only for scenes that take the BVH path (the tiny-scene records are built from the leaf order as a permutation of the triangles)
    const bool spatial = opt.split_alpha > 0.0 && nt > kSmallSceneMaxTris && wtri != nullptr;
    const float spatial_min = (float)(opt.split_alpha * (double)half_area(scene));
    const size_t ref_budget = (size_t)((double)nt * (1.0 + opt.split_budget)) + 8;
    size_t refs_total = nt;                                                       // references handed out so far (leaves made + still on the stack)
    std::vector<Task> tasks;
    const uint32_t cutoff = (!spatial && nt >= 65536u && opt.threads != 1) ? std::max<uint32_t>(4096u, nt / 256u) : 0u;
    const TopDown top_down{opt, wtri, spatial, spatial_min, ref_budget, cutoff, tasks};
    top_down(refs, 0u, tn, order, max_depth, refs_total, cutoff != 0u);
    sw.lap("top-down, serial part");
    if (!tasks.empty()) {
        run_tasks(top_down, tasks, opt.threads);
        sw.lap("top-down, tasks");
        splice_tasks(tasks, tn, order, max_depth);
        tasks.clear(); tasks.shrink_to_fit();
    }
    sw.lap("splice");
    // ---- insertion-based optimisation of the topology ----
    if (opt.reinsert_passes > 0 && tn.size() > 7) {
        std::vector<int32_t> parent(tn.size(), -1);
        for (size_t i = 0; i < tn.size(); i++) if (!tn[i].count) { parent[tn[i].left] = (int32_t)i; parent[tn[i].right] = (int32_t)i; }
        // a pass tries the nodes with the largest boxes: all of them on small trees, the top `reinsert_cap` on large ones (on the 3.8 M-triangle street the largest 10 % of the
        // nodes carry 5.4 of the 7 % a full pass takes off the shadow rays' node steps, at a seventh of its time)
        const double frac = std::min(opt.reinsert_frac, (double)opt.reinsert_cap / (double)tn.size());
        for (int pass = 0; pass < opt.reinsert_passes; pass++) reinsert_pass(tn, parent, frac);
        std::vector<std::pair<int32_t, uint32_t>> dst; dst.push_back({0, 0u}); max_depth = 0;
        while (!dst.empty()) { const auto it = dst.back(); dst.pop_back(); max_depth = std::max(max_depth, it.second); if (!tn[it.first].count) { dst.push_back({tn[it.first].left, it.second + 1}); dst.push_back({tn[it.first].right, it.second + 1}); } }
    }
    sw.lap("re-insertion");
}

// The TOP of a PLOC tree (host twin and GPU build alike): the top-down SAH builder and the re-insertion passes over the clusters PLOC stopped at, single clusters as leaves
// (a leaf the builder refuses to split becomes a chain).  out: root first; left / right >= 0: index into out, < 0: ~cluster index; boxes unpadded.
void build_cluster_top(const float* boxes6, uint32_t m, const BvhBuildOptions& opt_in, std::vector<ClusterTopNode>& out) {
    BvhBuildOptions opt = opt_in; opt.leaf_stop = 1; opt.split_alpha = 0.0; opt.ploc_radius = 0;
    std::vector<Ref> refs(m); Box scene = empty_box();
    for (uint32_t i = 0; i < m; i++) { for (int a = 0; a < 3; a++) { refs[i].box.mn[a] = boxes6[(size_t)i * 6 + a]; refs[i].box.mx[a] = boxes6[(size_t)i * 6 + 3 + a]; } refs[i].tri = i; grow(scene, refs[i].box); }
    const std::vector<Ref> cref = refs;                                         // (the builder consumes its reference stack)
    std::vector<TmpNode> tn; std::vector<uint32_t> order; uint32_t depth = 0;
    BuildStopwatch quiet("", 0, false);
    build_tmp_tree(refs, scene, opt, tn, order, depth, quiet, nullptr);
    out.clear();
    if (m == 0) return;
    struct It { int32_t src, dst; };
    std::vector<It> st; out.emplace_back(); st.push_back({0, 0});
    auto setbox = [](ClusterTopNode& N, const Box& b) { for (int a = 0; a < 3; a++) { N.mn[a] = b.mn[a]; N.mx[a] = b.mx[a]; } };
    while (!st.empty()) {
        const It it = st.back(); st.pop_back();
        const TmpNode T = tn[it.src];
        if (!T.count) {
            setbox(out[it.dst], T.box);
            int32_t child[2];
            for (int w = 0; w < 2; w++) {
                const int32_t c = w ? T.right : T.left;
                if (tn[c].count == 1) child[w] = ~(int32_t)order[tn[c].first];
                else { child[w] = (int32_t)out.size(); out.emplace_back(); st.push_back({c, child[w]}); }
            }
            out[it.dst].left = child[0]; out[it.dst].right = child[1];
            continue;
        }
        // a leaf of k >= 2 clusters (or the root as a leaf): a chain  (c0, (c1, (c2, ...)))
        const uint32_t f = T.first, k = T.count;
        if (k == 1) { setbox(out[it.dst], T.box); out[it.dst].left = ~(int32_t)order[f]; out[it.dst].right = ~(int32_t)order[f]; continue; }      // (m == 1: the caller does not call)
        int32_t at = it.dst;
        for (uint32_t q = 0; q + 1 < k; q++) {
            Box rest = empty_box(); for (uint32_t z = q; z < k; z++) grow(rest, cref[order[f + z]].box);
            setbox(out[at], rest);
            out[at].left = ~(int32_t)order[f + q];
            if (q + 2 == k) out[at].right = ~(int32_t)order[f + q + 1];
            else { const int32_t nx = (int32_t)out.size(); out.emplace_back(); out[at].right = nx; at = nx; }
        }
    }
}

// PLOC (the GPU build's bottom-up half, restated on the host): bottom-up clusters, then the top of the tree — over <= ploc_top clusters, with single clusters as leaves —
// by the top-down builder and the re-insertion passes (build_cluster_top), and the clusters' subtrees hung in below.  The top of a tree is where every ray passes
// (5.7 of 12.4 node steps in the first three wide levels on the atrium): it gets the expensive builder, the bottom the parallel one.
static void build_ploc_tree(const std::vector<Ref>& refs, const Box& scene, const BvhBuildOptions& opt, std::vector<TmpNode>& tn, std::vector<uint32_t>& order, uint32_t& max_depth, BuildStopwatch& sw) {
    std::vector<PlocNode> pool; std::vector<int32_t> cl;
    ploc_clusters(refs, scene, opt.ploc_radius, std::max(1u, opt.ploc_top), pool, cl);
    sw.lap("ploc clusters");
    if (cl.size() == 1) { tn.emplace_back(); ploc_expand(pool, cl[0], 0, 0u, tn, order, max_depth); }
    else {
        std::vector<float> boxes(cl.size() * 6);
        for (size_t i = 0; i < cl.size(); i++) for (int a = 0; a < 3; a++) { boxes[i * 6 + a] = pool[cl[i]].box.mn[a]; boxes[i * 6 + 3 + a] = pool[cl[i]].box.mx[a]; }
        std::vector<ClusterTopNode> top; build_cluster_top(boxes.data(), (uint32_t)cl.size(), opt, top);
        sw.lap("ploc top");
        struct It { int32_t src, dst; uint32_t depth; };
        std::vector<It> st; tn.emplace_back(); st.push_back({0, 0, 0u});
        while (!st.empty()) {
            const It it = st.back(); st.pop_back();
            const ClusterTopNode N = top[it.src];
            for (int a = 0; a < 3; a++) { tn[it.dst].box.mn[a] = N.mn[a]; tn[it.dst].box.mx[a] = N.mx[a]; }
            const int32_t l = (int32_t)tn.size(); tn.emplace_back(); const int32_t r = (int32_t)tn.size(); tn.emplace_back();
            tn[it.dst].left = l; tn[it.dst].right = r; tn[it.dst].count = 0;
            // (right first on the stack so that the left subtree is expanded first: leaf order = depth-first left to right)
            if (N.right >= 0) st.push_back({N.right, r, it.depth + 1});
            if (N.left >= 0) st.push_back({N.left, l, it.depth + 1});
            if (N.left < 0) ploc_expand(pool, cl[~N.left], l, it.depth + 1, tn, order, max_depth);
            if (N.right < 0) ploc_expand(pool, cl[~N.right], r, it.depth + 1, tn, order, max_depth);
        }
    }
    sw.lap("ploc expand");
}

// ---- leaf order: depth-first, left to right, so that every subtree owns ONE contiguous range of references (collapse_bvh8 merges small subtrees into a
//      leaf slot by range; the build emits the right side first and the re-insertion moves subtrees) ----
static void depth_first_leaf_order(std::vector<TmpNode>& tn, std::vector<uint32_t>& order) {
    std::vector<uint32_t> emitted; emitted.reserve(order.size());
    std::vector<int32_t> dfs; dfs.push_back(0);
    while (!dfs.empty() && !tn.empty()) {
        const int32_t i = dfs.back(); dfs.pop_back();
        if (tn[i].count) { const uint32_t f = tn[i].first; tn[i].first = (uint32_t)emitted.size(); for (uint32_t k = 0; k < tn[i].count; k++) emitted.push_back(order[f + k]); }
        else if (tn[i].left >= 0) { dfs.push_back(tn[i].right); dfs.push_back(tn[i].left); }
    }
    if (emitted.size() == order.size()) order.swap(emitted);
}

// ---- breadth-first relayout with children boxes stored in the parent ----
static void layout_breadth_first(const std::vector<TmpNode>& tn, uint32_t nt, float pad_abs, std::vector<NodeGPU>& nodes) {
    nodes.clear();
    auto enc_leaf = [](const TmpNode& n) -> int32_t { return (int32_t)~((n.first << 3) | (n.count - 1)); };
    auto put_box = [&](NodeGPU& N, int which, const Box* b) {
        float mn[3], mx[3];
        for (int a = 0; a < 3; a++) { mn[a] = b ? b->mn[a] - pad_abs : INFINITY; mx[a] = b ? b->mx[a] + pad_abs : -INFINITY; }
        if (which == 0) { N.a = {mn[0], mn[1], mn[2], mx[0]}; N.b.x = mx[1]; N.b.y = mx[2]; }
        else { N.b.z = mn[0]; N.b.w = mn[1]; N.c = {mn[2], mx[0], mx[1], mx[2]}; }
    };
    if (nt == 0) {
        NodeGPU N{}; put_box(N, 0, nullptr); put_box(N, 1, nullptr);
        N.d = {u2f((uint32_t)kEmptyChild), u2f((uint32_t)kEmptyChild), 0.0f, 0.0f};
        nodes.push_back(N); return;
    }
    if (tn[0].count) {   // root is a leaf: wrap it
        NodeGPU N{}; put_box(N, 0, &tn[0].box); put_box(N, 1, nullptr);
        N.d = {u2f((uint32_t)enc_leaf(tn[0])), u2f((uint32_t)kEmptyChild), 0.0f, 0.0f};
        nodes.push_back(N); return;
    }
    std::vector<int32_t> bfs; bfs.push_back(0);            // internal nodes only
    for (size_t h = 0; h < bfs.size(); h++) {
        const TmpNode& n = tn[bfs[h]];
        if (!tn[n.left].count) bfs.push_back(n.left);
        if (!tn[n.right].count) bfs.push_back(n.right);
    }
    // second pass needs the final indices of children: recompute in the same order
    nodes.resize(bfs.size());
    {
        std::vector<int32_t> idx_of(tn.size(), -1);
        for (size_t h = 0; h < bfs.size(); h++) idx_of[bfs[h]] = (int32_t)h;
        for (size_t h = 0; h < bfs.size(); h++) {
            const TmpNode& n = tn[bfs[h]];
            NodeGPU N{};
            put_box(N, 0, &tn[n.left].box); put_box(N, 1, &tn[n.right].box);
            int32_t c0 = tn[n.left].count ? enc_leaf(tn[n.left]) : idx_of[n.left];
            int32_t c1 = tn[n.right].count ? enc_leaf(tn[n.right]) : idx_of[n.right];
            N.d = {u2f((uint32_t)c0), u2f((uint32_t)c1), 0.0f, 0.0f};
            nodes[h] = N;
        }
    }
}

void build_bvh(const std::vector<float>& wtri, float pad_abs, std::vector<NodeGPU>& nodes, std::vector<uint32_t>& order, uint32_t& max_depth, const BvhBuildOptions& opt) {
    const uint32_t nt = (uint32_t)(wtri.size() / 9);
    BuildStopwatch sw("[build]   bvh2: ", 20);
    std::vector<Ref> refs(nt);
    Box scene = empty_box();
    for (uint32_t i = 0; i < nt; i++) {
        const float* t = &wtri[(size_t)i * 9];
        for (int a = 0; a < 3; a++) {
            refs[i].box.mn[a] = std::min(t[a], std::min(t[3 + a], t[6 + a]));
            refs[i].box.mx[a] = std::max(t[a], std::max(t[3 + a], t[6 + a]));
        }
        refs[i].tri = i;
        grow(scene, refs[i].box);
    }
    order.clear(); order.reserve(nt);
    std::vector<TmpNode> tn; tn.reserve((size_t)2 * nt + 2);
    max_depth = 0;
    const bool ploc = opt.ploc_radius > 0 && nt > kSmallSceneMaxTris;
    if (ploc) build_ploc_tree(refs, scene, opt, tn, order, max_depth, sw);
    else build_tmp_tree(refs, scene, opt, tn, order, max_depth, sw, wtri.data());
    depth_first_leaf_order(tn, order);
    sw.lap("leaf order");
    layout_breadth_first(tn, nt, pad_abs, nodes);
}

}  // namespace rtx

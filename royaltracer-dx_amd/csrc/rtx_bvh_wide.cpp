// rtx_bvh_wide.cpp — binary tree -> compressed 8-wide device form (collapse_bvh8, the permuted leaf triangles) and the coverage validators of the wide tree.
// No HIP calls in this file.
#include "rtx_scene_host.hpp"
#include "rtx_wide.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace rtx {

// Compressed 8-wide collapse.  Which binary subtrees become wide nodes or leaf slots is chosen by a surface-area-heuristic
// dynamic program (below).  The child boxes
// are the binary tree's padded boxes rounded OUTWARD onto the node's byte grid (checked in exact double arithmetic), so the
// wide tree is conservative whenever the binary one is.
bool collapse_bvh8(const std::vector<NodeGPU>& n2, std::vector<Node8GPU>& n8, std::vector<uint32_t>& tri_slots, uint32_t& max_stack,
                   std::vector<uint32_t>* level_start, const BvhBuildOptions& opt) {
    struct Ch { float mn[3], mx[3]; int32_t c; };
    auto get = [](const NodeGPU& N, int which) {
        Ch r;
        if (which == 0) { r.mn[0] = N.a.x; r.mn[1] = N.a.y; r.mn[2] = N.a.z; r.mx[0] = N.a.w; r.mx[1] = N.b.x; r.mx[2] = N.b.y; r.c = (int32_t)f2u(N.d.x); }
        else            { r.mn[0] = N.b.z; r.mn[1] = N.b.w; r.mn[2] = N.c.x; r.mx[0] = N.c.y; r.mx[1] = N.c.z; r.mx[2] = N.c.w; r.c = (int32_t)f2u(N.d.y); }
        return r;
    };
    auto area = [](const Ch& b) { const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2]; return dx * dy + dy * dz + dz * dx; };
    n8.clear(); tri_slots.clear(); max_stack = 0;
    if (level_start) level_start->clear();
    if (n2.empty()) return true;
    // ---- which binary subtrees become wide nodes / leaf slots: surface-area-heuristic dynamic program (Ylitie et al. 2017,
    //      section 3.1).  cost[n][i] = cheapest way to represent binary subtree n with at most i child slots of its wide
    //      parent: as ONE slot (a leaf slot holding all its <= 4 triangles, or an internal slot = a wide node of its own with 8
    //      slots to distribute), or split between its two children.  Greedy "open the largest child" filled 4.1 of 8 slots. ----
    const size_t nn = n2.size();
    // a triangle test is 95 VALU instructions against ~200 of a node step, but triangle steps run with half the lanes of node steps
    // (profiles/r02_traversal.md), so per ray it costs more than the 0.45 the instruction counts say: measured k_trace_closest
    // 23.80 / 21.31 ms (C3 / C5) at 0.45, 23.39 / 20.93 at 0.7, 23.49 / 21.00 at 1.0, 23.53 / 20.95 at 1.5, 24.30 / 21.82 at 0.3
    const double kNodeCost = 1.0, kTriCost = opt.tri_cost;
    // (the program itself, the gathering of a wide node's children and the greedy slot assignment live in rtx_wide.hpp: the GPU build runs the same code)
    struct Sub { uint32_t first; };
    std::vector<Sub> sub(nn);
    std::vector<WideDp> dp(nn);
    auto is_leaf = [](int32_t c) { return c < 0; };
    auto leaf_cnt = [](int32_t c) { return ((~(uint32_t)c) & 7u) + 1u; };
    auto leaf_first = [](int32_t c) { return (~(uint32_t)c) >> 3; };
    auto wb = [](const Ch& c) { WBox b; for (int a = 0; a < 3; a++) { b.mn[a] = c.mn[a]; b.mx[a] = c.mx[a]; } return b; };
    for (size_t n = nn; n-- > 0;) {
        const Ch L = get(n2[n], 0), R = get(n2[n], 1);
        if (L.c == kEmptyChild || R.c == kEmptyChild) {      // only the root may have an unused child (scenes with < 2 leaves)
            if (n != 0) return false;
            sub[n] = Sub{0u}; memset(&dp[n], 0, sizeof(WideDp)); continue;
        }
        if ((L.c >= 0 && (size_t)L.c <= n) || (R.c >= 0 && (size_t)R.c <= n) || (L.c >= 0 && (size_t)L.c >= nn) || (R.c >= 0 && (size_t)R.c >= nn)) return false;
        const WideDpChild dl{area(L), is_leaf(L.c) ? leaf_cnt(L.c) : 0u, is_leaf(L.c) ? nullptr : &dp[(size_t)L.c]}, dr{area(R), is_leaf(R.c) ? leaf_cnt(R.c) : 0u, is_leaf(R.c) ? nullptr : &dp[(size_t)R.c]};
        wide_dp_combine(dl, dr, wbox_area(wbox_union(wb(L), wb(R))), kNodeCost, kTriCost, dp[n]);
        sub[n] = Sub{is_leaf(L.c) ? leaf_first(L.c) : sub[(size_t)L.c].first};
    }
    // children of the wide node made from binary node x, following the recorded decisions
    struct Acc {
        const std::vector<NodeGPU>& n2; const std::vector<Sub>& sub; const std::vector<WideDp>& dp; decltype(get)& get_;
        bool is_leaf(const Ch& c) const { return c.c < 0; }
        void children(const Ch& c, Ch& L, Ch& R) const { L = get_(n2[(size_t)c.c], 0); R = get_(n2[(size_t)c.c], 1); }
        uint8_t choice(const Ch& c, int i) const { return dp[(size_t)c.c].choice[i]; }
        Ch merged(const Ch& c) const { Ch r = c; r.c = (int32_t)~((sub[(size_t)c.c].first << 3) | (dp[(size_t)c.c].prims - 1u)); return r; }      // a leaf slot holding the subtree's <= 4 triangles (contiguous in leaf order)
    };
    const Acc acc{n2, sub, dp, get};
    std::vector<int32_t> src; src.push_back(0);            // binary node behind each wide node, breadth-first
    for (size_t h = 0; h < src.size(); h++) {
        Ch ch[8]; int m = 0;
        const NodeGPU& N = n2[(size_t)src[h]];
        {
            const Ch L = get(N, 0), R = get(N, 1);
            if (L.c == kEmptyChild || R.c == kEmptyChild) { if (L.c != kEmptyChild) ch[m++] = L; if (R.c != kEmptyChild) ch[m++] = R; }
            else { bool internal[8]; m = wide_children(acc, L, R, (int)dp[(size_t)src[h]].choice[8], ch, internal); }
            if (m > 8) return false;
        }
        Node8GPU W{};
        float bmn[3] = {0, 0, 0}, bmx[3] = {0, 0, 0};
        // ---- slots: child with the largest projection on an octant's diagonal gets that octant's slot (greedy assignment) ----
        int slot_of[8]; bool slot_used[8] = {false, false, false, false, false, false, false, false};
        {
            WBox cb[8]; for (int k = 0; k < m; k++) cb[k] = wb(ch[k]);
            wide_assign_slots(cb, m, bmn, bmx, slot_of);           // (node bounds + the greedy assignment)
            if (opt.slot_assign == 0) { for (int k = 0; k < m; k++) slot_used[slot_of[k]] = true; }
            else {
                double cost[8][8];
                for (int k = 0; k < m; k++) for (int sl = 0; sl < 8; sl++) {
                    double c = 0.0;
                    for (int a = 0; a < 3; a++) {
                        const double rel = 0.5 * ((double)ch[k].mn[a] + (double)ch[k].mx[a]) - 0.5 * ((double)bmn[a] + (double)bmx[a]);
                        c += ((sl >> a) & 1) ? rel : -rel;
                    }
                    cost[k][sl] = c;
                }
                // the assignment that maximises the summed projections (Ylitie et al. solve it by auction; with eight slots a subset table is exact): best[k][S] = children
                // k.. placed into the free slots of S
                double best[9][256]; int8_t pick[9][256];
                for (int S = 0; S < 256; S++) best[m][S] = 0.0;
                for (int k = m - 1; k >= 0; k--) for (int S = 0; S < 256; S++) {
                    best[k][S] = -1e300; pick[k][S] = -1;
                    if (__builtin_popcount(S) != k) continue;                       // S = slots taken by children 0..k-1
                    for (int sl = 0; sl < 8; sl++) if (!(S & (1 << sl))) {
                        const double nxt = best[k + 1][S | (1 << sl)];
                        if (nxt <= -1e299 && k + 1 < m) continue;
                        const double c = cost[k][sl] + (k + 1 < m ? nxt : 0.0);
                        if (c > best[k][S]) { best[k][S] = c; pick[k][S] = (int8_t)sl; }
                    }
                }
                int S = 0;
                for (int k = 0; k < m; k++) { const int sl = pick[k][S]; slot_of[k] = sl; slot_used[sl] = true; S |= 1 << sl; }
            }
        }
        int child_at[8]; for (int sl = 0; sl < 8; sl++) child_at[sl] = -1;
        for (int k = 0; k < m; k++) child_at[slot_of[k]] = k;
        // ---- byte grid per axis: smallest power of two with 255 steps covering the node ----
        W.px = bmn[0]; W.py = bmn[1]; W.pz = bmn[2];
        int eb[3]; double step[3];
        for (int a = 0; a < 3; a++) {
            const double ext = (double)bmx[a] - (double)bmn[a];
            int e = -120;
            if (ext > 0.0) { e = std::max(-120, (int)std::ilogb(ext / 255.0)); while (std::ldexp(255.0, e) < ext) e++; }
            if (e > 120 || !std::isfinite(ext)) return false;
            eb[a] = e + 127; step[a] = std::ldexp(1.0, e);
        }
        uint32_t imask = 0, trivalid = 0;
        uint8_t qb[6][8];
        for (int sl = 0; sl < 8; sl++) {
            for (int r = 0; r < 6; r++) qb[r][sl] = 0;
            const int k = child_at[sl];
            if (k < 0) continue;
            const float p[3] = {W.px, W.py, W.pz};
            for (int a = 0; a < 3; a++) {
                double qlo = std::floor(((double)ch[k].mn[a] - (double)p[a]) / step[a]), qhi = std::ceil(((double)ch[k].mx[a] - (double)p[a]) / step[a]);
                qlo = std::min(255.0, std::max(0.0, qlo)); qhi = std::min(255.0, std::max(0.0, qhi));
                // exact check: the decoded planes bracket the source box
                if ((double)p[a] + qlo * step[a] > (double)ch[k].mn[a] || (double)p[a] + qhi * step[a] < (double)ch[k].mx[a]) return false;
                qb[a][sl] = (uint8_t)qlo; qb[3 + a][sl] = (uint8_t)qhi;
            }
            if (ch[k].c >= 0) imask |= 1u << sl;
        }
        W.child_base = (uint32_t)src.size();
        for (int sl = 0; sl < 8; sl++) if (imask & (1u << sl)) src.push_back(ch[child_at[sl]].c);
        W.tri_base = (uint32_t)tri_slots.size();
        for (int sl = 0; sl < 8; sl++) {
            const int k = child_at[sl];
            if (k < 0 || ch[k].c >= 0) continue;
            const uint32_t v = ~(uint32_t)ch[k].c, first = v >> 3, cnt = (v & 7u) + 1u;
            if (cnt > 4) return false;
            trivalid |= ((1u << cnt) - 1u) << (4 * sl);
            for (uint32_t t = 0; t < cnt; t++) tri_slots.push_back(first + t);
        }
        W.e_imask = (uint32_t)eb[0] | (uint32_t)eb[1] << 8 | (uint32_t)eb[2] << 16 | imask << 24;
        W.trivalid = trivalid; W.pad = 0;
        for (int r = 0; r < 6; r++) {
            W.q[2 * r]     = (uint32_t)qb[r][0] | (uint32_t)qb[r][1] << 8 | (uint32_t)qb[r][2] << 16 | (uint32_t)qb[r][3] << 24;
            W.q[2 * r + 1] = (uint32_t)qb[r][4] | (uint32_t)qb[r][5] << 8 | (uint32_t)qb[r][6] << 16 | (uint32_t)qb[r][7] << 24;
        }
        n8.push_back(W);
        if (n8.size() >= (1u << 28)) return false;
    }
    std::vector<uint32_t> need(n8.size(), 0);                // children have larger indices: one reverse sweep
    for (size_t i = n8.size(); i-- > 0;) {
        const uint32_t imask = n8[i].e_imask >> 24, nint = (uint32_t)__builtin_popcount(imask);
        uint32_t deep = 0;
        for (uint32_t r = 0; r < nint; r++) deep = std::max(deep, need[(size_t)n8[i].child_base + r]);
        need[i] = (nint > 1 ? 1u : 0u) + deep;
    }
    max_stack = need[0];
    if (level_start) {                                       // breadth-first order: a level is a contiguous index range
        std::vector<uint32_t> level(n8.size(), 0);
        for (size_t i = 0; i < n8.size(); i++) {
            const uint32_t nint = (uint32_t)__builtin_popcount(n8[i].e_imask >> 24);
            for (uint32_t r = 0; r < nint; r++) level[(size_t)n8[i].child_base + r] = level[i] + 1;
        }
        for (size_t i = 0; i < n8.size(); i++) {
            if (i && level[i] < level[i - 1]) return false;
            if (i == 0 || level[i] != level[i - 1]) level_start->push_back((uint32_t)i);
        }
        level_start->push_back((uint32_t)n8.size());
    }
    return true;
}

void leaf_triangles(const std::vector<float>& wtri, const std::vector<uint32_t>& leaf_order, std::vector<TriGPU>& tris) {
    tris.resize(leaf_order.size());
    for (size_t s = 0; s < leaf_order.size(); s++) tris[s] = leaf_triangle(&wtri[(size_t)leaf_order[s] * 9], leaf_order[s]);
}

bool wide_from_binary(BuiltScene& B, const BvhBuildOptions& opt) {
    if (!collapse_bvh8(B.nodes, B.nodes8, B.tri_slots8, B.stack8, &B.level_start8, opt)) return false;
    B.tris8.resize(B.tri_slots8.size());
    for (size_t i = 0; i < B.tri_slots8.size(); i++) B.tris8[i] = B.tris[B.tri_slots8[i]];
    return true;
}

// Coverage bookkeeping shared by the validators of the binary and of the wide tree.  A triangle referenced ONCE must lie inside every box above its
// reference (all three corners).  A triangle that spatial splits handed to several leaves is checked on 28 points (corners, edge thirds, an interior lattice):
// each must lie inside all boxes above ONE of the references — the property the traversal needs (a hit point is found through whichever reference's boxes
// contain it).  Points are evaluated in double; the tolerance covers that evaluation only (boxes of split parts are rounded outward by a float spacing).
CoverCheck::CoverCheck(const std::vector<float>& world_tris9) : w(world_tris9), refs((uint32_t)(world_tris9.size() / 9), 0u) {}
void CoverCheck::count(uint32_t g) { refs[g]++; }
int CoverCheck::add(uint32_t g, const double mn[3], const double mx[3]) {
    if (refs[g] == 1) {
        for (int vtx = 0; vtx < 3; vtx++) for (int a = 0; a < 3; a++) { const double c = w[(size_t)g * 9 + vtx * 3 + a]; if (c < mn[a] || c > mx[a]) return 16; }
        return 0;
    }
    boxes.push_back({g, {mn[0], mn[1], mn[2], mx[0], mx[1], mx[2]}});
    return 0;
}
int CoverCheck::finish() {
    for (uint32_t r : refs) if (!r) return 17;
    std::stable_sort(boxes.begin(), boxes.end(), [](const Part& a, const Part& b) { return a.tri < b.tri; });
    for (size_t i = 0; i < boxes.size();) {
        size_t j = i; while (j < boxes.size() && boxes[j].tri == boxes[i].tri) j++;
        const float* t = &w[(size_t)boxes[i].tri * 9];
        double scale = 1.0; for (int k = 0; k < 9; k++) scale = std::max(scale, std::fabs((double)t[k]));
        const double tol = 1e-12 * scale;
        for (int a = 0; a <= 6; a++) for (int b = 0; a + b <= 6; b++) {
            const double u = a / 6.0, v = b / 6.0, q = 1.0 - u - v;
            const double pt[3] = {q * t[0] + u * t[3] + v * t[6], q * t[1] + u * t[4] + v * t[7], q * t[2] + u * t[5] + v * t[8]};
            bool in = false;
            for (size_t k = i; k < j && !in; k++) { const double* bx = boxes[k].b; in = pt[0] >= bx[0] - tol && pt[1] >= bx[1] - tol && pt[2] >= bx[2] - tol && pt[0] <= bx[3] + tol && pt[1] <= bx[4] + tol && pt[2] <= bx[5] + tol; }
            if (!in) return 24;
        }
        i = j;
    }
    return 0;
}

// the compressed 8-wide collapse: same coverage properties, checked on the DECODED byte-grid boxes of the wide nodes
int validate_bvh8(const std::vector<float>& w, const std::vector<Node8GPU>& nodes, const std::vector<uint32_t>& order,
                  const std::vector<uint32_t>& tri_slots, uint32_t* max_stack_seen, const std::vector<uint8_t>* hidden, double pad_abs) {
    const uint32_t ntris = (uint32_t)(w.size() / 9), nrefs = (uint32_t)tri_slots.size();
    if (order.size() != nrefs || nrefs < ntris) return 20;
    struct It { uint32_t node; double mn[3], mx[3]; uint32_t pushes; };
    std::vector<uint8_t> used(nrefs, 0), visited(nodes.size(), 0);
    if (nodes.empty()) return ntris ? 10 : 0;
    CoverCheck cover(w);
    for (uint32_t s = 0; s < nrefs; s++) { if (tri_slots[s] >= nrefs || order[tri_slots[s]] >= ntris) return 14; cover.count(order[tri_slots[s]]); }
    const double inf = INFINITY;
    // hidden entries: the bounds of the VISIBLE triangles below every node, bottom-up (children have larger indices than their parent), and the slack a decoded box may have
    struct VBox { double mn[3], mx[3]; };
    std::vector<VBox> vis;
    double slack = 0.0;
    if (hidden) {
        if (hidden->size() != nrefs) return 20;
        double scale = 1.0; for (float c : w) scale = std::max(scale, std::fabs((double)c));
        slack = pad_abs + 1e-6 * scale;
        vis.assign(nodes.size(), VBox{{inf, inf, inf}, {-inf, -inf, -inf}});
        for (size_t n = nodes.size(); n-- > 0;) {
            const Node8GPU& N = nodes[n];
            const uint32_t imask = N.e_imask >> 24;
            uint32_t rank = 0, tri_at = N.tri_base;
            for (int sl = 0; sl < 8; sl++) {
                const uint32_t nib = (N.trivalid >> (4 * sl)) & 0xfu;
                if ((imask >> sl) & 1u) {
                    const uint32_t c = N.child_base + rank++;
                    if (c <= n) return 12;
                    if (c >= nodes.size()) return 13;
                    for (int a = 0; a < 3; a++) { vis[n].mn[a] = std::min(vis[n].mn[a], vis[c].mn[a]); vis[n].mx[a] = std::max(vis[n].mx[a], vis[c].mx[a]); }
                } else for (uint32_t k = 0; k < (uint32_t)__builtin_popcount(nib); k++, tri_at++) {
                    if (tri_at >= nrefs) return 14;
                    if ((*hidden)[tri_at]) continue;
                    const float* t = &w[(size_t)order[tri_slots[tri_at]] * 9];
                    for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) { vis[n].mn[a] = std::min(vis[n].mn[a], (double)t[v * 3 + a]); vis[n].mx[a] = std::max(vis[n].mx[a], (double)t[v * 3 + a]); }
                }
            }
        }
    }
    std::vector<It> st;
    st.push_back({0u, {-inf, -inf, -inf}, {inf, inf, inf}, 0u});
    uint32_t deepest = 0;
    while (!st.empty()) {
        const It it = st.back(); st.pop_back();
        if (it.node >= nodes.size()) return 13;
        if (visited[it.node]) return 11;
        visited[it.node] = 1;
        const Node8GPU& N = nodes[it.node];
        const double p[3] = {N.px, N.py, N.pz};
        double step[3];
        for (int a = 0; a < 3; a++) { const int eb = (int)((N.e_imask >> (8 * a)) & 0xffu); if (eb < 1 || eb > 254) return 21; step[a] = std::ldexp(1.0, eb - 127); }
        const uint32_t imask = N.e_imask >> 24;
        const uint32_t nint = (uint32_t)__builtin_popcount(imask);
        const uint32_t pushes = it.pushes + (nint > 1 ? 1u : 0u);
        deepest = std::max(deepest, pushes);
        uint32_t rank = 0, tri_at = N.tri_base;
        for (int sl = 0; sl < 8; sl++) {
            const uint32_t nib = (N.trivalid >> (4 * sl)) & 0xfu;
            const bool internal = (imask >> sl) & 1u;
            if (internal && nib) return 22;
            if (!internal && !nib) continue;
            double mn[3], mx[3];
            bool quantised_empty = true;
            for (int a = 0; a < 3; a++) {
                const uint32_t qlo = (N.q[2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu, qhi = (N.q[2 * (3 + a) + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu;
                mn[a] = std::max(p[a] + qlo * step[a], it.mn[a]); mx[a] = std::min(p[a] + qhi * step[a], it.mx[a]);
                quantised_empty = quantised_empty && qlo == 255u && qhi == 0u;
            }
            if (hidden) {                                                        // what the child's box may cover: the visible triangles below it
                VBox need{{inf, inf, inf}, {-inf, -inf, -inf}};
                if (internal) { const uint32_t c = N.child_base + rank; if (c >= nodes.size()) return 13; need = vis[c]; }
                else for (uint32_t k = 0, s = tri_at; k < (uint32_t)__builtin_popcount(nib) && s < nrefs; k++, s++) {
                    if ((*hidden)[s]) continue;
                    const float* t = &w[(size_t)order[tri_slots[s]] * 9];
                    for (int v = 0; v < 3; v++) for (int a = 0; a < 3; a++) { need.mn[a] = std::min(need.mn[a], (double)t[v * 3 + a]); need.mx[a] = std::max(need.mx[a], (double)t[v * 3 + a]); }
                }
                if (need.mn[0] > need.mx[0]) { if (!quantised_empty) return 25; }
                else for (int a = 0; a < 3; a++) {
                    const uint32_t qlo = (N.q[2 * a + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu, qhi = (N.q[2 * (3 + a) + (sl >> 2)] >> (8 * (sl & 3))) & 0xffu;
                    if (p[a] + qlo * step[a] < need.mn[a] - slack - 2.0 * step[a] || p[a] + qhi * step[a] > need.mx[a] + slack + 2.0 * step[a]) return 26;
                }
            }
            if (internal) {
                const uint32_t c = N.child_base + rank++;
                if (c <= it.node) return 12;                                     // breadth-first: children after parents
                It nx; nx.node = c; nx.pushes = pushes;
                for (int a = 0; a < 3; a++) { nx.mn[a] = mn[a]; nx.mx[a] = mx[a]; }
                st.push_back(nx);
            } else {
                if (nib != 1 && nib != 3 && nib != 7 && nib != 15) return 23;
                const uint32_t cnt = (uint32_t)__builtin_popcount(nib);
                for (uint32_t k = 0; k < cnt; k++, tri_at++) {
                    if (tri_at >= nrefs) return 14;
                    if (used[tri_at]) return 15;                                 // every leaf entry belongs to one leaf slot
                    used[tri_at] = 1;
                    if (hidden && (*hidden)[tri_at]) continue;                   // in its slot, exempt from containment: no ray may find it
                    if (int r = cover.add(order[tri_slots[tri_at]], mn, mx)) return r;
                }
            }
        }
    }
    for (uint32_t i = 0; i < nrefs; i++) if (!used[i]) return 17;
    for (size_t i = 0; i < nodes.size(); i++) if (!visited[i]) return 18;
    if (int r = cover.finish()) return r;
    if (max_stack_seen) *max_stack_seen = deepest;
    return 0;
}

}  // namespace rtx

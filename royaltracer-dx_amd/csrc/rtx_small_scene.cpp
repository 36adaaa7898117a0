// rtx_small_scene.cpp — the tiny-scene path (<= kSmallSceneMaxTris triangles, e.g. the Cornell Box): triangles merged into planar convex quads, the conservative pre-test
// records of rtx_types.hpp (SmallRecPair), which of them are faces of the scene's convex hull, and the per-triangle guard of that shortcut (TriShade::guard_tau).
// No HIP calls in this file.
#include "rtx_scene_host.hpp"
#include <algorithm>
#include <array>
#include <cmath>

namespace rtx {

namespace {
struct D3 { double x, y, z; };
inline D3 sub(D3 a, D3 b) { return D3{a.x - b.x, a.y - b.y, a.z - b.z}; }
inline D3 crs(D3 a, D3 b) { return D3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline double dt(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline D3 nrm(D3 a) { double l = sqrt(dt(a, a)); return l > 0 ? D3{a.x / l, a.y / l, a.z / l} : D3{0, 0, 0}; }
inline bool same(D3 a, D3 b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
using TriVerts = std::vector<std::array<D3, 3>>;       // the scene's triangles in leaf order, in double
struct Rec { double pl[4]; double e[4][4]; int s0, s1; double pv[4][3]; };     // pv: polygon vertices (a triangle repeats its last one)

Rec make_rec(const std::vector<D3>& poly, D3 nu, int s0, int s1) {
    Rec R; R.s0 = s0; R.s1 = s1;
    for (int k = 0; k < 4; k++) { const D3& q = poly[std::min<size_t>((size_t)k, poly.size() - 1)]; R.pv[k][0] = q.x; R.pv[k][1] = q.y; R.pv[k][2] = q.z; }
    R.pl[0] = nu.x; R.pl[1] = nu.y; R.pl[2] = nu.z; R.pl[3] = dt(nu, poly[0]);
    for (int k = 0; k < 4; k++) { R.e[k][0] = R.e[k][1] = R.e[k][2] = 0.0; R.e[k][3] = 1e30; }     // always inside
    for (size_t k = 0; k < poly.size(); k++) {
        D3 A = poly[k], Bv = poly[(k + 1) % poly.size()];
        D3 m = nrm(crs(nu, sub(Bv, A)));                     // in-plane, pointing inside for a polygon wound CCW about nu
        R.e[k][0] = m.x; R.e[k][1] = m.y; R.e[k][2] = m.z; R.e[k][3] = -dt(m, A);
    }
    return R;
}

// one record per planar convex quad of two triangles sharing an edge, or per triangle that finds no partner
std::vector<Rec> merge_quads(const TriVerts& V, double tol, float scale) {
    const size_t n = V.size();
    std::vector<Rec> recs; std::vector<uint8_t> used(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (used[i]) continue;
        used[i] = 1;
        D3 ni = crs(sub(V[i][1], V[i][0]), sub(V[i][2], V[i][0]));
        const double nn = sqrt(dt(ni, ni));
        if (!(nn > 0.0)) {                                       // zero-area triangle: the exact test always rejects it
            Rec R; R.s0 = (int)i; R.s1 = -1; for (int k = 0; k < 4; k++) { R.pl[k] = 0; R.e[k][0] = R.e[k][1] = R.e[k][2] = 0; R.e[k][3] = -1e30; R.pv[k][0] = V[i][0].x; R.pv[k][1] = V[i][0].y; R.pv[k][2] = V[i][0].z; }
            recs.push_back(R); continue;
        }
        D3 nu = nrm(ni);
        int partner = -1; std::vector<D3> quad;
        for (size_t j = i + 1; j < n && partner < 0; j++) {
            if (used[j]) continue;
            for (int a = 0; a < 3 && partner < 0; a++) {         // apex of i = vertex a, shared edge (a+1, a+2)
                D3 r = V[i][a], pp = V[i][(a + 1) % 3], q = V[i][(a + 2) % 3];
                for (int bb = 0; bb < 3; bb++) {
                    D3 sA = V[j][bb], j1 = V[j][(bb + 1) % 3], j2 = V[j][(bb + 2) % 3];
                    if (!((same(j1, pp) && same(j2, q)) || (same(j1, q) && same(j2, pp)))) continue;
                    if (fabs(dt(nu, sub(sA, r))) > tol) continue;                       // coplanar
                    std::vector<D3> poly = {r, pp, sA, q};                                // around the quad, CCW about nu
                    bool convex = true;
                    for (int k = 0; k < 4 && convex; k++) {
                        D3 m = nrm(crs(nu, sub(poly[(k + 1) % 4], poly[k])));
                        for (int v = 0; v < 4; v++) if (dt(m, sub(poly[v], poly[k])) < -1e-7 * (double)scale) { convex = false; break; }
                    }
                    if (!convex) continue;
                    partner = (int)j; quad = poly; break;
                }
            }
        }
        if (partner >= 0) { used[partner] = 1; recs.push_back(make_rec(quad, nu, (int)i, partner)); }
        else recs.push_back(make_rec({V[i][0], V[i][1], V[i][2]}, nu, (int)i, -1));
    }
    return recs;
}

// Per-ray guard of the shortcut.  An NEE segment may skip the hull faces only if its ORIGIN lies clearly inside every hull
// plane: a shading point in a room corner can sit within rounding distance of the neighbouring wall's plane, whose triangles the
// float test then accepts for a segment grazing that wall (expected about once per 1080p x 64 spp Cornell frame).
//   origin = pos + s_bias n_T (n_T: the shading normal the kernels compute, flat shading here), so for triangle T and hull plane B
//   dist(origin, B) = dist(pos, B) + s_bias (n_T . n_B), n_B the plane's inward normal;  required >= safety (20 x the float
//   error of pos), i.e.  dist(pos, B) >= s_TB := safety - s_bias (n_T . n_B).  Planes with s_TB <= 0 never matter (T's own plane,
//   the other half of a slightly twisted wall: the origin is s_bias inside them wherever it is on T).
//   dist(pos, B) is the barycentric blend of T's vertex distances d_i(B) >= 0, hence >= min(b) max_i d_i(B):
//   tau_T = max over the planes that matter of s_TB / max_i d_i(B), and "min barycentric >= tau_T" proves the origin safe.
// Three instructions per hit (TriShade::guard_tau); a wave with a ray that fails runs its shadow rays against all records.
void set_guard_tau(BuiltScene& B, const TriVerts& V, const std::vector<Rec>& hull) {
    const size_t n = V.size();
    const double safety = (double)B.small_hull_margin;
    for (size_t si = 0; si < n && !hull.empty(); si++) {
        const uint32_t g = f2u(B.tris[si].v0.w);
        if (g >= B.shade.size()) continue;
        const TriShade& ts = B.shade[g];
        const f3 nw = normalize(xform_dir(B.insts[ts.inst].nrm, mk3(ts.flat[0], ts.flat[1], ts.flat[2])));      // = Surf::normal of a flat-shaded hit (rtx_shade.hpp)
        double tau = 0.0;
        for (const Rec& Hf : hull) {
            double dmax = 0.0, side = 0.0;
            for (size_t s2 = 0; s2 < n; s2++) for (int k = 0; k < 3; k++) {                                     // the scene's side of the plane
                const double dd = Hf.pl[0] * V[s2][k].x + Hf.pl[1] * V[s2][k].y + Hf.pl[2] * V[s2][k].z - Hf.pl[3];
                if (fabs(dd) > fabs(side)) side = dd;
            }
            const double sgn = side >= 0.0 ? 1.0 : -1.0;
            for (int k = 0; k < 3; k++) dmax = std::max(dmax, fabs(Hf.pl[0] * V[si][k].x + Hf.pl[1] * V[si][k].y + Hf.pl[2] * V[si][k].z - Hf.pl[3]));
            const double ndot = sgn * (Hf.pl[0] * (double)nw.x + Hf.pl[1] * (double)nw.y + Hf.pl[2] * (double)nw.z);
            const double need = safety - (double)kSBias * ndot + 1e-7 * (double)kSBias;                            // (+ rounding of n_T)
            if (!(need > 0.0)) continue;
            tau = dmax > 0.0 ? std::max(tau, need / dmax) : 2.0;
        }
        B.shade[g].guard_tau = (float)std::min(2.0, tau * 1.000001);
    }
}

// Faces of the scene's convex hull last: a record whose plane has ALL scene vertices on one side (within tol) cannot lie
// strictly between two points of the scene, so NEE shadow segments (surface point + bias -> light point, shortened at both
// ends) only need the records before them.  In a closed room that is every wall: Cornell keeps 11 of its 17 records.
void hull_faces_last(BuiltScene& B, const TriVerts& V, double tol, float scale, std::vector<Rec>& recs) {
    const size_t n = V.size();
    // EMISSIVE records always stay in the occluder list: an NEE segment ENDS on a light, a margin of 1e-4 short of it, and for a long
    // grazing segment the float Moeller-Trumbore t of the light's own triangle is off by more than that, so the brute-force
    // definition (and the oracle) reports the light as its own occluder.  Found by the analytic rectangle-light test, whose light is
    // a hull face; the Cornell light hangs below the ceiling and was in the list anyway.
    auto emissive = [&](int slot) {
        if (slot < 0) return false;
        const uint32_t g = f2u(B.tris[(size_t)slot].v0.w);
        const uint32_t m = g < B.shade.size() ? B.shade[g].mat : 0xFFFFFFFFu;
        return m < B.mats.size() && B.mats[m].Ke_len > 0.0f;
    };
    // The same holds for a hull face whose PLANE carries a light vertex (a lamp flush with a wall or ceiling): the segment's end point
    // lies in that plane, so the face's triangles can pass the float test too.  Such faces stay in the list as well.
    std::vector<D3> light_verts;
    for (size_t s = 0; s < n; s++) if (emissive((int)s)) for (int k = 0; k < 3; k++) light_verts.push_back(V[s][k]);
    const double near_plane = 5.0 * (double)kSBias + 2e-4 * (double)scale;      // the segment's end margin + the float test's error of t (Cornell's light hangs 9e-4 below its ceiling: not near)
    // The shortcut also needs FLAT shading everywhere: the segment starts at pos + bias * SHADING normal and is only cast when the
    // shading normal faces the light; with interpolated vertex normals neither keeps it on the inner side of the face it starts
    // on (brute force then reports that face as the occluder).  Any smooth-shaded triangle turns the shortcut off for the scene.
    // ... and it needs room for the per-ray guard (traverse_small): the origin sits s_bias inside its OWN face, which must stay
    // outside the guard's margin, or every ray would fall back anyway.
    bool all_flat = B.small_hull_margin < 0.9f * kSBias;
    for (const TriShade& ts : B.shade) for (int k = 0; k < 3; k++)
        if (ts.n0[k] != ts.flat[k] || ts.n1[k] != ts.flat[k] || ts.n2[k] != ts.flat[k]) all_flat = false;
    std::vector<Rec> occ, hull;
    for (const Rec& R : recs) {
        if (!all_flat) { occ.push_back(R); continue; }
        bool pos = false, neg = false;
        const bool degenerate = R.pl[0] == 0.0 && R.pl[1] == 0.0 && R.pl[2] == 0.0;
        bool light = emissive(R.s0) || emissive(R.s1);
        for (const D3& q : light_verts) if (fabs(R.pl[0] * q.x + R.pl[1] * q.y + R.pl[2] * q.z - R.pl[3]) <= near_plane) light = true;
        for (size_t s = 0; s < n && !degenerate; s++) for (int k = 0; k < 3; k++) {
            const double dd = R.pl[0] * V[s][k].x + R.pl[1] * V[s][k].y + R.pl[2] * V[s][k].z - R.pl[3];
            if (dd > tol) pos = true; else if (dd < -tol) neg = true;
        }
        (((pos && neg) || light) ? occ : hull).push_back(R);
    }
    B.small_nocc = (uint32_t)occ.size();
    set_guard_tau(B, V, hull);
    recs = occ; recs.insert(recs.end(), hull.begin(), hull.end());
}

// ---- slab form of a quad record (SmallSlabPair, rtx_types.hpp) ----
// CONSERVATIVENESS.  The pre-test may only drop a record whose exact test rejects the ray, and the argument for the edge planes is: the exact test accepts only plane points P
// within r = delta + mt of the polygon (delta: the fixed distance tolerance, mt: the per-ray margin of rtx_traverse.hpp), and ANY half-plane that contains the polygon, moved
// outward by r, contains every point within r of the polygon.  That argument never uses that the half-plane is an EDGE of the polygon.  A slab lo <= w . P <= hi with
// lo = min and hi = max of w . v over the corners is two such half-planes (|w| = 1, so r is a distance along w), hence  h + delta - |w . P - c| >= -mt  with c the slab's centre
// and h its half-width is as conservative as  m . P + c_k + delta >= -mt  for two opposite edges at once.  Two slabs along two adjacent edge normals bound the quad by a
// parallelogram: the same region for a parallelogram, slightly more (`excess`) for a near-parallelogram — and more only ever forwards more rays to the exact test.  Which
// records take this form (kSlabTau) is therefore a COST choice, never a correctness condition.
// Float evaluation: centre and half-width are taken over the corners with the directions and the centre AS ROUNDED TO FLOAT, so the float coefficients bound the polygon exactly;
// the device's three products, three sums and the final subtraction err by at most 7 x 2^-24 of (sum |w_i P_i| + |c| + h) for P near the polygon, covered by `pad`
// (2e-6 of that magnitude, 30 x 2^-24), and h is rounded upward.
constexpr double kSlabTau = 0.02;             // a quad whose bounding parallelogram exceeds its area by more than this keeps its four edge planes
struct Slab { bool quad = false; double excess = -1.0; float w[2][3] = {{0, 0, 0}, {0, 0, 0}}, c[2] = {0, 0}, h[2] = {-1e30f, -1e30f}; };     // default: never inside (padding record)
Slab slab_of_quad(const Rec& R, double delta) {
    Slab S;
    if (R.s1 < 0) return S;                                   // a single triangle (or a zero-area one): no slab form
    D3 p[4]; for (int k = 0; k < 4; k++) p[k] = D3{R.pv[k][0], R.pv[k][1], R.pv[k][2]};
    const D3 nu{R.pl[0], R.pl[1], R.pl[2]};
    const double area = 0.5 * fabs(dt(crs(sub(p[2], p[0]), sub(p[3], p[1])), nu));
    if (!(area > 0.0)) return S;
    int best_k = -1; double best = 0.0;
    for (int k = 0; k < 4; k++) {                             // the bounding parallelogram along each pair of ADJACENT edge normals: the smallest one
        double width[2];
        for (int s = 0; s < 2; s++) {
            const double* m = R.e[(k + s) & 3];
            double lo = 1e300, hi = -1e300;
            for (int v = 0; v < 4; v++) { const double q = m[0] * p[v].x + m[1] * p[v].y + m[2] * p[v].z; lo = std::min(lo, q); hi = std::max(hi, q); }
            width[s] = hi - lo;
        }
        const double* m0 = R.e[k]; const double* m1 = R.e[(k + 1) & 3];
        const double sn = fabs(dt(crs(D3{m0[0], m0[1], m0[2]}, D3{m1[0], m1[1], m1[2]}), nu));
        if (!(sn > 1e-9)) continue;
        const double ex = width[0] * width[1] / sn / area - 1.0;
        if (best_k < 0 || ex < best) { best_k = k; best = ex; }
    }
    if (best_k < 0) return S;
    S.quad = true; S.excess = std::max(best, 0.0);
    for (int s = 0; s < 2; s++) {
        const double* m = R.e[(best_k + s) & 3];
        for (int a = 0; a < 3; a++) S.w[s][a] = (float)m[a];
        double lo = 1e300, hi = -1e300, mag = 0.0;
        for (int v = 0; v < 4; v++) {
            const double q = (double)S.w[s][0] * p[v].x + (double)S.w[s][1] * p[v].y + (double)S.w[s][2] * p[v].z;
            lo = std::min(lo, q); hi = std::max(hi, q);
            mag = std::max(mag, fabs((double)S.w[s][0] * p[v].x) + fabs((double)S.w[s][1] * p[v].y) + fabs((double)S.w[s][2] * p[v].z));
        }
        S.c[s] = (float)(0.5 * (lo + hi));
        const double half = std::max(hi - (double)S.c[s], (double)S.c[s] - lo);          // about the ROUNDED centre
        const double pad = 2e-6 * (mag + fabs((double)S.c[s]) + half + delta);
        S.h[s] = std::nextafterf((float)(half + delta + pad), INFINITY);
    }
    return S;
}

// the device form of the records: their triangles, their polygon corners, and the plane / edge coefficients two records to a SmallRecPair
void pack_records(BuiltScene& B, const std::vector<Rec>& recs, double delta) {
    B.small_nrec = (uint32_t)recs.size();
    B.small_tris.assign(((recs.size() + 1) & ~(size_t)1) * 2, TriGPU{{0, 0, 0, u2f(kMissPrim)}, {0, 0, 0, 0}, {0, 0, 0, 0}});   // the padding record of an odd count owns two zero-area triangles
    const TriGPU none{{0, 0, 0, u2f(kMissPrim)}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    for (size_t r = 0; r < recs.size(); r++) { B.small_tris[2 * r] = B.tris[recs[r].s0]; B.small_tris[2 * r + 1] = recs[r].s1 >= 0 ? B.tris[recs[r].s1] : none; }
    // polygon corners per record: the primary-ray kernel culls records against the pyramid of each 8x8 pixel block
    B.small_poly.assign(((recs.size() + 1) & ~(size_t)1) * 4, F4{0.0f, 0.0f, 0.0f, 0.0f});
    for (size_t r = 0; r < recs.size(); r++) for (int k = 0; k < 4; k++) B.small_poly[r * 4 + k] = {(float)recs[r].pv[k][0], (float)recs[r].pv[k][1], (float)recs[r].pv[k][2], 0.0f};
    for (size_t r = 0; r < recs.size(); r += 2) {
        SmallRecPair P;
        for (int e = 0; e < 2; e++) {
            const bool have = r + e < recs.size();
            for (int row = 0; row < 20; row++) {
                double v;
                if (!have) v = (row == 7 || row == 11 || row == 15 || row == 19) ? -1e30 : 0.0;       // padding: never inside
                else v = row < 4 ? recs[r + e].pl[row] : recs[r + e].e[(row - 4) / 4][(row - 4) % 4] + ((row - 4) % 4 == 3 ? delta : 0.0);   // edge constants carry the distance tolerance
                P.r[row][e] = (float)v;
            }
        }
        B.small_recs.push_back(P);
    }
    // the slab table: a pair is a slab pair when BOTH its records are quads within kSlabTau (the padding record of an odd count qualifies: its slabs are never inside)
    B.small_excess.assign(recs.size(), -1.0f);
    for (size_t r = 0; r < recs.size(); r += 2) {
        SmallSlabPair Q; bool both = true;
        for (int e = 0; e < 2; e++) {
            const bool have = r + e < recs.size();
            const Slab S = have ? slab_of_quad(recs[r + e], delta) : Slab{};
            if (have) { B.small_excess[r + e] = (float)S.excess; both = both && S.quad && S.excess <= kSlabTau; }
            for (int s = 0; s < 2; s++) { for (int a = 0; a < 3; a++) Q.r[5 * s + a][e] = S.w[s][a]; Q.r[5 * s + 3][e] = S.c[s]; Q.r[5 * s + 4][e] = S.h[s]; }
        }
        if (both) B.small_slab_mask |= 1u << (r / 2);
        B.small_slabs.push_back(Q);
    }
}
}  // namespace

// ---- tiny scenes: merge triangles into planar convex quads and build the conservative pre-test records ----
void build_small_scene(BuiltScene& B, const std::vector<float>& wtri, float scale) {
    const std::vector<uint32_t>& leaf_order = B.leaf_order;
    B.small_recs.clear(); B.small_tris.clear(); B.small_poly.clear(); B.small_slabs.clear(); B.small_excess.clear(); B.small_slab_mask = 0; B.small_nrec = 0; B.small_nocc = 0;
    if (leaf_order.empty() || leaf_order.size() > kSmallSceneMaxTris) return;
    const double delta = 2e-5 * (double)scale, tol = 1e-6 * (double)scale;
    B.small_delta = (float)delta; B.small_cm = 4e-6f * scale; B.small_hull_margin = 2e-6f * scale;     // how far inside every hull plane an NEE origin must lie (20 x the float error of a hit position)
    const size_t n = leaf_order.size();
    TriVerts V(n);
    for (size_t s = 0; s < n; s++) { const float* t = &wtri[(size_t)leaf_order[s] * 9]; for (int k = 0; k < 3; k++) V[s][k] = D3{t[k * 3], t[k * 3 + 1], t[k * 3 + 2]}; }
    std::vector<Rec> recs = merge_quads(V, tol, scale);
    hull_faces_last(B, V, tol, scale, recs);
    pack_records(B, recs, delta);
}

}  // namespace rtx

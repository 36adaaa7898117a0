"""The slab form of the tiny-scene pre-test records (csrc/rtx_small_scene.cpp: slab_of_quad; csrc/rtx_traverse.hpp: traverse_small) on the CPU: a float32 numpy twin of the
device's inequality, in the device's operation order, over the brute-force hits of the oracle.  The pre-test may only discard a record whose exact test rejects the ray."""
import numpy as np
import pytest

import small_slab_scenes as S

F = np.float32


def fma(a, b, c):
    """a * b + c rounded once (the product of two float32 is exact in float64)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def plane_point(R, rays):
    """rows 0-3 of the records R (n, 20) at the rays (n, 8), float32, as the `pair` body of traverse_small computes them -> nd, t, P, mt (cm is applied by the caller)"""
    o, d = rays[:, 0:3].astype(F), rays[:, 4:7].astype(F)
    nd = fma(R[:, 2], d[:, 2], fma(R[:, 1], d[:, 1], R[:, 0] * d[:, 0]))
    no = R[:, 3] - fma(R[:, 2], o[:, 2], fma(R[:, 1], o[:, 1], R[:, 0] * o[:, 0]))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ind = F(1.0) / nd
        t = no * ind
        P = [fma(t, d[:, k], o[:, k]) for k in range(3)]
    return nd, ind, t, P


def pretest(recs, slabs, cm, rays, rec, form):
    """the verdict of the pre-test for record rec[i] at ray i: (accepted by the inequality, forwarded by the grazing rule).  form: per ray, True = slab, False = edge planes"""
    R, Q = recs[rec].astype(F), slabs[rec].astype(F)
    nd, ind, t, (px, py, pz) = plane_point(R, rays)
    with np.errstate(invalid="ignore", over="ignore"):
        mt = fma(np.abs(ind), F(cm), np.abs(t) * F(1e-5))
        a0 = (t + mt) - rays[:, 3].astype(F); a1 = (rays[:, 7].astype(F) + mt) - t
        a = fma(Q[:, 2], pz, fma(Q[:, 1], py, Q[:, 0] * px)) - Q[:, 3]
        b = fma(Q[:, 7], pz, fma(Q[:, 6], py, Q[:, 5] * px)) - Q[:, 8]
        me_slab = np.fmin(Q[:, 4] - np.abs(a), Q[:, 9] - np.abs(b))
        e = [fma(R[:, 6 + 4 * k], pz, fma(R[:, 5 + 4 * k], py, R[:, 4 + 4 * k] * px)) + R[:, 7 + 4 * k] for k in range(4)]
        me_edge = np.fmin(e[0], np.fmin(np.fmin(e[1], e[2]), e[3]))
        me = np.where(form, me_slab, me_edge)
        ok = (a0 >= 0) & (a1 >= 0) & (me >= -mt)
    return ok, np.abs(nd) < F(1e-3)


def cornell_shapes(scene, ids):
    """Cornell's records as Shapes: the quad of a record pair of triangles in the host's corner order (apex, shared edge start, the partner's apex, shared edge end)"""
    v, idx, _ = scene.meshes[0]
    P = v[:, :3].astype(np.float64); tri = np.asarray(idx).reshape(-1, 3)
    sh = S.Shapes()
    for i, j in ids:
        if j < 0:
            sh.tri(P[tri[i]]); continue
        shared = [a for a in tri[i] if any(np.array_equal(P[a], P[b]) for b in tri[j])]
        apex_i = [a for a in tri[i] if a not in shared][0]
        apex_j = [b for b in tri[j] if not any(np.array_equal(P[b], P[a]) for a in shared)][0]
        k = list(tri[i]).index(apex_i)
        sh.quad([P[apex_i], P[tri[i][(k + 1) % 3]], P[apex_j], P[tri[i][(k + 2) % 3]]])
    return sh


def cornell_mix(rt, orc, cornell):
    """the ray mix of test_tiny_scene_pretest_records_are_conservative (tests/test_host_layer.py)"""
    o = orc.Oracle().load(cornell, 16 / 9)
    rng = np.random.default_rng(3)
    n = 60000
    r = np.zeros((n, 8), np.float32); r[:, 0:3] = rng.uniform(-0.2, 1.2, (n, 3)); d = rng.normal(size=(n, 3)); r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3], r[:, 7] = 1e-4, 1e4
    cam = o.primary_rays(rt.Params(width=160, height=90)); hc = o.trace_closest(cam, 1); hitc = hc.view(np.uint32)[:, 3] != 0xFFFFFFFF
    sec = np.zeros((int(hitc.sum()), 8), np.float32); sec[:, 0:3] = cam[hitc, 0:3] + hc[hitc, 0:1] * cam[hitc, 4:7]
    d = rng.normal(size=(len(sec), 3)); sec[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True); sec[:, 3], sec[:, 7] = 2e-5, 1e4
    graz = r[:8000].copy(); graz[:, 5] = rng.uniform(-2e-4, 2e-4, len(graz)); graz[:, 4:7] /= np.linalg.norm(graz[:, 4:7], axis=1, keepdims=True)
    return o, np.concatenate([cam, r, sec, graz])


@pytest.fixture(scope="module")
def scenes(rt, tmp_path_factory):
    return S.all_scenes(rt, tmp_path_factory.mktemp("slabs"))


def check_scene(name, scene, shapes, o, rays):
    recs, ids, _, cm = scene.small_records()
    slabs, excess, mask = scene.small_slabs()
    nrec = len(recs)
    pair_is_slab = np.array([(mask >> (r // 2)) & 1 for r in range(nrec)], bool)
    quad = excess >= 0
    # the kind of a pair: both records quads within TAU (the padding record of an odd count qualifies)
    for kp in range((nrec + 1) // 2):
        both = all(r >= nrec or (quad[r] and excess[r] <= S.TAU) for r in (2 * kp, 2 * kp + 1))
        assert bool((mask >> kp) & 1) == both, (name, kp)
    assert mask >> ((nrec + 1) // 2) == 0
    assert (quad == (ids[:, 1] >= 0)).all(), name
    h = o.trace_closest(rays, 0); prim = h.view(np.uint32)[:, 3]; hit = prim != 0xFFFFFFFF
    ntri = int(ids.max()) + 1
    owner = np.full(ntri, -1); owner[ids[:, 0]] = np.arange(nrec); two = ids[:, 1] >= 0; owner[ids[two, 1]] = np.arange(nrec)[two]
    rec = owner[prim[hit]]
    assert (rec >= 0).all()
    hr = rays[hit]
    # 1. the form the device runs (slab pairs by their slabs, the others by their edge planes) keeps every true hit
    ok, graz = pretest(recs, slabs, cm, hr, rec, pair_is_slab[rec])
    assert (ok | graz).all(), f"{name}: {int((~(ok | graz)).sum())} true hits would be discarded by the pre-test"
    # 2. the slab inequality on EVERY quad, also those beyond TAU (tau is a cost knob, not a correctness condition), and how many hits it decides itself
    on_quad = quad[rec]
    ok_s, graz_s = pretest(recs, slabs, cm, hr[on_quad], rec[on_quad], np.ones(int(on_quad.sum()), bool))
    assert (ok_s | graz_s).all(), f"{name}: {int((~(ok_s | graz_s)).sum())} true hits would be discarded by the slab form"
    decided = float(ok_s.mean()) if on_quad.any() else 1.0
    # 3. (ray, record) pairs over all rays and all quads: what the slab form forwards and the edge form drops
    more = total = 0
    for r in np.nonzero(quad)[0]:
        rr = np.full(len(rays), r)
        s_ok, g = pretest(recs, slabs, cm, rays, rr, np.ones(len(rays), bool))
        e_ok, _ = pretest(recs, slabs, cm, rays, rr, np.zeros(len(rays), bool))
        more += int((s_ok & ~e_ok & ~g).sum()); total += len(rays)
        lost = int((e_ok & ~s_ok & ~g).sum())          # the slabs' h carries a rounding pad above delta: nothing the edge form accepts may be dropped on a parallelogram
        if excess[r] == 0.0:
            assert lost == 0, (name, int(r), lost)
    print(f"{name}: {int(hit.sum())} hits of {len(rays)} rays, {int(on_quad.sum())} on quads, decided by the slab inequality {100 * decided:.2f} %, "
          f"slab accepts / edge rejects {more} of {total} (ray, quad) pairs = {100.0 * more / max(total, 1):.4f} %")
    return decided, int(on_quad.sum())


def test_cornell_excess_and_kinds(cornell):
    """the bounding parallelograms of the Cornell quads against the float64 figures, the host's against this file's own computation, and the kind of every pair"""
    recs, ids, _, _ = cornell.small_records()
    slabs, excess, mask = cornell.small_slabs()
    sh = cornell_shapes(cornell, ids)
    mine = [S.quad_excess(q) for q in sh.quads]
    host = excess[excess >= 0]
    assert len(mine) == len(host) == 15 and (excess < 0).sum() == 2
    assert np.allclose(host, mine, rtol=0, atol=1e-6)
    want = [0.0] * 11 + [0.0029, 0.0038, 0.0058, 0.0115]
    # The figures were worked out to 0.01 %, so one unit of their last digit is the bound.  (Half a unit would not do for the tall block's top: the smallest of its four
    # bounding parallelograms exceeds it by 0.3746 %, the one along its last two edge normals by 0.3756 %, which is the 0.38 % of the list.)
    assert np.allclose(np.sort(host), want, rtol=0, atol=1e-4), np.sort(host)
    assert np.sort(host)[:11].max() < 1e-6
    assert bin(mask).count("1") == 7 and mask == 0b110011111                        # 7 of the 9 pairs; the two with a single triangle of the twisted wall stay generic
    # the slab of a quad bounds its corners (float coefficients, float64 evaluation), the distance tolerance on top
    for q, r in zip(sh.quads, np.nonzero(excess >= 0)[0]):
        for s in (0, 5):
            a = q @ slabs[r, s:s + 3].astype(np.float64) - float(slabs[r, s + 3])
            assert np.abs(a).max() <= float(slabs[r, s + 4]) - 1.9e-5


def test_cornell_mix_is_conservative(rt, orc, cornell):
    o, rays = cornell_mix(rt, orc, cornell)
    recs, ids, _, _ = cornell.small_records()
    aimed = S.aimed_rays(cornell_shapes(cornell, ids), np.random.default_rng(5), per=24)
    decided, n = check_scene("cornell", cornell, None, o, np.concatenate([rays, aimed]))
    assert n > 40000
    assert decided >= 0.85, f"only {100 * decided:.2f} % of the hits are decided by the slab inequality itself"


@pytest.mark.parametrize("name", ["rects", "perturbed"] + ["records%d" % n for n in S.RECORD_COUNTS])
def test_generated_scenes_are_conservative(rt, orc, scenes, name):
    scene, shapes = scenes[name]
    rng = np.random.default_rng(len(name) * 131 + 7)
    rays = np.concatenate([S.random_rays(12000, rng), S.aimed_rays(shapes, rng)])
    graz = S.random_rays(1000, rng); graz[:, 6] = rng.uniform(-2e-4, 2e-4, len(graz)); graz[:, 4:7] /= np.linalg.norm(graz[:, 4:7], axis=1, keepdims=True)
    decided, n = check_scene(name, scene, shapes, orc.Oracle().load(scene, 16 / 9), np.concatenate([rays, graz]))
    if n:
        assert decided >= 0.85, f"only {100 * decided:.2f} % of the hits are decided by the slab inequality itself"


def test_perturbed_quads_straddle_tau(scenes):
    """the kites built just below and just above TAU land on either side of it in the host's table, and the trapezoid far above"""
    scene, shapes = scenes["perturbed"]
    _, excess, _ = scene.small_slabs()
    host = np.sort(excess[excess >= 0])
    mine = np.sort([S.quad_excess(q) for q in shapes.quads])
    assert np.allclose(host, mine, rtol=0, atol=1e-5)
    assert ((host > 0.9 * S.TAU) & (host <= S.TAU)).sum() == 1 and ((host > S.TAU) & (host < 1.1 * S.TAU)).sum() == 1
    assert (excess < 0).sum() == 2 and host.max() > 0.15

"""CPU suite, part 2: the host layer (scene loader / material / camera API mirroring the reference) and
the C-ABI library itself (loads, exports every declared symbol, refuses to run without a GPU)."""
import ctypes
import glob
import json
import os
import re
import subprocess
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- loader pinned against the reference's vendored tinyobjloader (fixtures from oracle/ref_probe.cpp) ----
def expected_load(ref, material_offset, vertex_offset):
    """ObjLoader::loadObjFile (ObjLoader.h:393-495) re-derived in numpy from the raw tinyobj parse."""
    v = ref["vertices"].reshape(-1, 3); n = ref["normals"].reshape(-1, 3)
    verts, index, seen = [], [], {}
    for vi, ni in zip(ref["vertex_index"], ref["normal_index"]):
        pos = tuple(v[vi].tolist())
        nrm = tuple(n[ni].tolist()) if ni >= 0 else (0.0, 0.0, 0.0)
        if pos not in seen:                      # de-duplicated by POSITION only (Vertex.h:31-33)
            seen[pos] = len(verts); verts.append(pos + nrm + (float(vertex_offset),))
        index.append(seen[pos])
    matids = np.repeat(ref["material_ids"] + material_offset + 1, 3).astype(np.uint32)
    return np.array(verts, np.float32), np.array(index, np.uint32), matids


@pytest.fixture(scope="module")
def garage(rt, golden_dir):
    return rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")


def test_obj_loader_matches_tinyobj(rt, garage, golden_dir):
    mat_off, id_off = 0, 0
    for k, name in enumerate(("garage", "monke")):
        ref = np.load(os.path.join(golden_dir, f"ref_tinyobj_{name}.npz"))
        assert (ref["num_face_vertices"] == 3).all()
        ev, ei, em = expected_load(ref, mat_off, id_off)
        gv, gi, gm = garage.meshes[k]
        assert np.array_equal(bits(gv), bits(ev)), name
        assert np.array_equal(gi, ei) and np.array_equal(gm, em), name
        # material table: default first, then the model's materials (ObjLoader.h:415-444)
        d = garage.materials[mat_off]
        assert list(d[:4]) == [1, 1, 1, 1] and list(d[4:8]) == [1, 1, 1, 1] and list(d[12:16]) == [1, 0, 0, 0] and not d[16:].any()
        for j, m in enumerate(ref["materials"]):
            g = garage.materials[mat_off + 1 + j]
            assert np.array_equal(bits(g[0:3]), bits(m[0:3])) and g[3] == m[9]          # Kd, dissolve
            assert np.array_equal(bits(g[4:7]), bits(m[3:6])) and g[7] == 1.0           # Ks; Ni is never filled by the loader
            assert np.array_equal(bits(g[8:11]), bits(m[6:9]))                          # Ke
            assert np.array_equal(bits(g[12:16]), bits(m[10:14]))                       # Pr Pm Ps Pc
            assert (g[16:] > 0).all() and (g[16:] <= 1.0 + 1e-3).all()                  # Ess LUT
        mat_off += 1 + len(ref["materials"]); id_off += len(em)
    assert len(garage.materials) == 6 and garage.num_triangles == 1254 + 967
    mesh, m = garage.instances[1]                                                        # Renderer.cpp:444-449
    assert mesh == 1 and abs(m[0] - np.cos(1.57)) < 1e-6 and abs(m[2] + np.sin(1.57)) < 1e-6 and abs(m[8] - np.sin(1.57)) < 1e-6


def test_obj_loader_matches_tinyobj_on_random_files(rt, golden_dir):
    """24 random OBJ / MTL files (tests/golden/objfuzz, written by make_obj_fuzz.py together with what the reference's vendored
    tinyobjloader v2.0.0 parses from them): index forms incl. negative indices, quads, n-gons (tinyobj's ear clipping decides the order
    and the number of triangles), groups, CRLF / tabs / comments, unknown and missing materials, d vs Tr, the map_Kd default, PBR keys"""
    D = os.path.join(golden_dir, "objfuzz")
    ref = np.load(os.path.join(D, "ref.npz"))
    ngons = 0
    for k in range(24):
        r = {n: ref["f%02d_%s" % (k, n)] for n in ("vertices", "normals", "vertex_index", "normal_index", "material_ids", "num_face_vertices", "materials")}
        assert (r["num_face_vertices"] == 3).all()
        sc = rt.Scene.from_obj([os.path.join(D, "fz%02d.obj" % k)], D + "/")
        ev, ei, em = expected_load(r, 0, 0)
        gv, gi, gm = sc.meshes[0]
        assert gv.shape == ev.shape and np.array_equal(bits(gv), bits(ev)), k
        assert np.array_equal(gi, ei) and np.array_equal(gm, em), k
        assert len(sc.materials) == 1 + len(r["materials"]), k
        for j, m in enumerate(r["materials"]):
            g = sc.materials[1 + j]
            assert np.array_equal(bits(g[0:3]), bits(m[0:3])) and g[3] == m[9], (k, j)            # Kd (0.6 after a bare map_Kd), dissolve (d wins over Tr)
            assert np.array_equal(bits(g[4:7]), bits(m[3:6])) and np.array_equal(bits(g[8:11]), bits(m[6:9])), (k, j)   # Ks, Ke
            assert np.array_equal(bits(g[12:16]), bits(m[10:14])), (k, j)                          # Pr Pm Ps Pc
        with open(os.path.join(D, "fz%02d.obj" % k)) as f:
            ngons += sum(1 for line in f if line.startswith("f") and len(line.split()) > 5)
    assert ngons >= 10                                    # the set does exercise the ear clipping


def test_lookat_matches_glm(rt, golden_dir):
    for case in json.load(open(os.path.join(golden_dir, "ref_glm_lookat.json"))):
        a = case["args"]
        got = rt.lookat(a[0:3], a[3:6], a[6:9])
        assert np.array_equal(bits(got), bits(np.array(case["matrix"], np.float32))), case


def test_perspective_matrix(rt):
    fov, asp, zn, zf = np.float32(60 * 3.141592654 / 180), np.float32(16 / 9), 0.1, 1000.0
    p = rt.perspective_fov_rh(fov, asp, zn, zf).reshape(4, 4).T        # -> math (row, col)
    h = 1.0 / np.tan(0.5 * float(fov)); fr = zf / (zn - zf)
    expect = np.array([[h / float(asp), 0, 0, 0], [0, h, 0, 0], [0, 0, fr, fr * zn], [0, 0, -1, 0]])
    assert np.allclose(p, expect, rtol=2e-6, atol=1e-7)


def test_inverse_and_half_match_the_oracle(rt, orc):
    rng = np.random.default_rng(2)
    for _ in range(20):
        m = rng.normal(size=16).astype(np.float32)
        assert np.array_equal(bits(rt.mat4_inverse(m)), bits(orc.mat4_inverse(m)))
    for x in [0.6, 0.73, 0.05, 17.0, 1e-6, 65519.0, 60000.0, -0.12345]:
        assert rt.half_round(x) == orc.half_round(x) == float(np.float32(np.float16(np.float32(x))))


def test_ess_lut_generator(rt):
    a, b = rt.generate_ess_lut(1.0), rt.generate_ess_lut(1.0)
    assert np.array_equal(a, b)                                        # fixed seed: reproducible (reference: random_device)
    assert (a > 0.2).all() and (a < 0.6).all()
    smooth = rt.generate_ess_lut(0.2)
    assert (smooth > 0.7).all() and (smooth[8:] > 0.99).all() and (smooth <= 1.001).all()   # smooth GGX loses almost no energy to single scatter


def test_cornell_scene(rt, orc, cornell):
    assert cornell.num_triangles == 32 and len(cornell.materials) == 5 and len(cornell.meshes) == 1
    v, idx, mid = cornell.meshes[0]
    assert (v[:, 3:6] == 0).all() and (v[:, 6] == 0).all()            # flat shading; materialIDs base 0
    assert (mid.reshape(-1, 3) == mid.reshape(-1, 3)[:, :1]).all()
    assert sorted(set(mid.tolist())) == [1, 2, 3, 4]
    o = orc.Oracle().load(cornell, 16 / 9)
    L = o.lights()
    assert len(L) == 2 and (L[:, 12:15] == [17, 12, 4]).all()
    # every camera-visible surface faces the camera (v6 has no face forwarding, Hit_v6.hlsl:56)
    rays = o.primary_rays(rt.Params(width=160, height=90), 1)
    hits = o.trace_closest(rays, 1)
    hit = hits.view(np.uint32)[:, 3] != 0xFFFFFFFF
    s = o.surface(rays, hits)
    assert ((s[hit, 4:7] * rays[hit, 4:7]).sum(1) < 0).all()
    assert np.allclose(np.linalg.norm(s[hit, 4:7], axis=1), 1.0, atol=1e-6)


def test_sponza_class_scene(rt):
    sc = rt.Scene.sponza_class(262144, 260)
    assert abs(sc.num_triangles - 262144) <= 0.01 * 262144
    assert len(sc.materials) == 13
    v, idx, mid = sc.meshes[0]
    tri = v[idx.reshape(-1, 3)][:, :, :3]
    assert np.isfinite(tri).all() and np.abs(tri).max() < 3.0
    w = tri.reshape(-1, 9)
    rc, nodes, depth, leaf = rt.bvh_check(w)
    assert rc == 0 and leaf <= 4 and depth < 60 and nodes >= len(w) // 8
    rc8, nodes8, stack8 = rt.bvh8_check(w)                              # the compressed 8-wide device form of the same tree
    assert rc8 == 0 and nodes8 < nodes // 2 and stack8 <= 24, (rc8, nodes8, stack8)
    sc2 = rt.Scene.sponza_class(262144, 260)
    assert np.array_equal(sc2.meshes[0][0], v)                          # deterministic


def test_bvh_builder_invariants(rt, cornell):
    v, idx, _ = cornell.meshes[0]
    rc, nodes, depth, leaf = rt.bvh_check(v[idx.reshape(-1, 3)][:, :, :3].reshape(-1, 9))
    assert rc == 0 and leaf <= 4 and nodes < 32
    rng = np.random.default_rng(9)
    for n in (1, 2, 3, 7, 100, 5000):
        c = rng.uniform(-1, 1, (n, 1, 3)); t = (c + rng.normal(scale=0.02, size=(n, 3, 3))).astype(np.float32)
        assert rt.bvh_check(t.reshape(-1, 9))[0] == 0
        assert rt.bvh8_check(t.reshape(-1, 9))[0] == 0
    same = np.tile(np.array([[0, 0, 0, 1, 0, 0, 0, 1, 0]], np.float32), (37, 1))     # 37 identical triangles
    assert rt.bvh_check(same)[0] == 0
    assert rt.bvh8_check(same)[0] == 0
    assert rt.bvh8_check(np.zeros((0, 9), np.float32))[0] == 0


BUILDER_DEFAULTS = {"bins": 16, "sweep": 0, "leaf_stop": 2, "split": 0.0, "split_budget": 0.3, "reinsert": 2, "reinsert_frac": 1.0, "reinsert_cap": 200000, "slot_assign": 0, "tri_cost": 0.7, "threads": 0}


@pytest.fixture
def builder_options(rt):
    """set BVH builder knobs for one test; the process-wide defaults are restored afterwards"""
    def apply(**kw):
        for k, v in kw.items():
            rt.bvh_option(k, v)
    yield apply
    for k, v in BUILDER_DEFAULTS.items():
        rt.bvh_option(k, v)


def _lab_soup(kind, n, rng):
    c = rng.uniform(-1, 1, (n, 1, 3))
    if kind == "needles":                # long thin triangles: the case spatial splits exist for
        a = rng.uniform(-1, 1, (n, 3)); d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.stack([a, a + 1.5 * d, a + 1.5 * d + rng.normal(scale=0.002, size=(n, 3))], axis=1).astype(np.float32)
    if kind == "mixed":                  # a few room-sized triangles over a carpet of small ones
        small = c[: n - 12] * np.array([1.0, 0.02, 1.0]) + rng.normal(scale=0.02, size=(n - 12, 3, 3))
        big = rng.uniform(-1.2, 1.2, (12, 3, 3))
        return np.concatenate([small, big]).astype(np.float32)
    return (c + rng.normal(scale=0.03, size=(n, 3, 3))).astype(np.float32)


def test_parallel_build_gives_the_serial_tree(rt, builder_options):
    """build_bvh cuts subtrees of at most max(4096, n / 256) references out of its top-down loop and builds them in a thread pool (scenes of >= 65 536 triangles), splices them
    back in cutting order and renumbers the nodes into the serial loop's creation order; the re-insertion passes select their candidates (largest boxes first, ties by index)
    by nth_element + sort instead of a full stable sort.  Neither may change the tree: the replayed traversal of 20 000 rays takes the same node steps and triangle tests, ray
    for ray, with 1, 3 and the default number of threads, and the validators accept it."""
    rng = np.random.default_rng(41)
    n = 90000
    c = rng.uniform(-1, 1, (n, 1, 3)) * np.array([4.0, 1.0, 4.0])
    t = (c + rng.normal(scale=0.03, size=(n, 3, 3))).astype(np.float32)
    t[::7] = np.round(t[::7] * 8) / 8                      # exact ties: coincident and grid-aligned triangles
    m = 20000
    org = rng.uniform(-4, 4, (m, 3)) * np.array([1.0, 0.3, 1.0]); d = rng.normal(size=(m, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((m, 8), np.float32); rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = org, 1e-5, d, 1e30
    out = []
    for threads in (1, 3, 0):
        builder_options(threads=threads)
        got, refs = rt.bvh_replay(t, rays)
        assert refs == n
        out.append(bits(got).tobytes())
    assert out[0] == out[1] == out[2]
    assert (bits(np.frombuffer(out[0], np.uint32).reshape(-1, 4))[:, 3] != 0xFFFFFFFF).mean() > 0.2
    rc8, nodes8, stack8 = rt.bvh8_check(t.reshape(-1, 9))
    assert rc8 == 0 and stack8 <= 30


@pytest.mark.parametrize("opts", [dict(), dict(reinsert=0), dict(split=1e-5, sweep=64), dict(split=1e-7, split_budget=2.0, reinsert=3), dict(bins=8, leaf_stop=1, slot_assign=1)],
                         ids=["default", "no_reinsert", "split_sweep", "split_heavy", "misc"])
@pytest.mark.parametrize("kind", ["random", "needles", "mixed"])
def test_builder_variants_keep_the_tree_valid_and_the_replayed_traversal_exact(rt, orc, builder_options, kind, opts):
    """Every builder knob (spatial splits, re-insertion, sweep SAH, slot assignment) changes the tree and never an answer: the validators accept the tree, and the
    device traversal replayed on the host returns the brute-force closest hit (minimum over all triangles, ties to the lowest id) of the oracle — also where a
    triangle is referenced from several leaves."""
    rng = np.random.default_rng(sum(map(ord, kind)) + len(opts))
    t = _lab_soup(kind, 3000, rng)
    builder_options(**opts)
    rc, nodes, depth, leaf = rt.bvh_check(t.reshape(-1, 9))
    assert rc == 0 and leaf <= 4, (rc, leaf)
    rc8, nodes8, stack8 = rt.bvh8_check(t.reshape(-1, 9))
    assert rc8 == 0 and stack8 <= 30, (rc8, stack8)
    m = 6000
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    org = rng.uniform(lo - 0.1, hi + 0.1, (m, 3)); d = rng.normal(size=(m, 3))
    pick = rng.integers(0, len(t), m // 2); w = rng.dirichlet((1, 1, 1), m // 2); w[: m // 8] = np.eye(3)[rng.integers(0, 3, m // 8)]
    d[: m // 2] = (t[pick] * w[:, :, None]).sum(1) - org[: m // 2]
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    # a sixth of the rays LIE IN the plane of a triangle (origin and direction are combinations of its edges): Moeller-Trumbore's 0 / 0 case
    k = m // 6; pl = rng.integers(0, len(t), k); T = t[pl].astype(np.float64)
    a = rng.normal(scale=3.0, size=(k, 2)); b = rng.normal(size=(k, 2))
    org[-k:] = T[:, 0] + a[:, :1] * (T[:, 1] - T[:, 0]) + a[:, 1:] * (T[:, 2] - T[:, 0])
    d[-k:] = b[:, :1] * (T[:, 1] - T[:, 0]) + b[:, 1:] * (T[:, 2] - T[:, 0])
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    rays = np.zeros((m, 8), np.float32); rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = org, 1e-5, d, 1e30

    class Soup:
        materials = np.zeros((2, 32), np.float32)
        def __init__(self, tris):
            n = len(tris); v = np.zeros((3 * n, 7), np.float32); v[:, 0:3] = tris.reshape(-1, 3)
            self.meshes = [(v, np.arange(3 * n, dtype=np.uint32), np.ones(3 * n, np.uint32))]
            self.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
        def view_proj(self, aspect):
            e = np.eye(4, dtype=np.float32).reshape(16); return e, e

    ref = orc.Oracle().load(Soup(t), 1.0).trace_closest(rays, mode=0)                 # brute force over all triangles
    got, refs = rt.bvh_replay(t, rays)
    if opts.get("split"):
        assert refs > len(t) or kind == "random", "spatial splits added no reference"
    else:
        assert refs == len(t)
    hit = bits(ref)[:, 3] != 0xFFFFFFFF
    assert hit.mean() > 0.3
    # EVERY ray: since round 5 the hit definition carries a determinant floor (csrc/rtx_math.hpp: tri_det_floor), so the 0 / 0 "hits" of rays lying in a sliver's plane, which
    # brute force reported and every tree culled, no longer exist and nothing is excluded from the comparison
    assert np.array_equal(bits(got)[:, 3], bits(ref)[:, 3]), "closest-hit triangle ids differ from brute force"
    assert np.array_equal(bits(got)[hit, 0], bits(ref)[hit, 0]), "closest-hit distances differ from brute force"
    # any-hit: the same answer in every visiting order
    sh = rays.copy(); sh[:, 7] = rng.uniform(0.05, 2.0, m).astype(np.float32)
    occ = [bits(rt.bvh_replay(t, sh, any_hit=True, any_order=k)[0])[:, 3] != 0xFFFFFFFF for k in (0, 1, 2)]
    assert np.array_equal(occ[0], occ[1]) and np.array_equal(occ[0], occ[2])
    assert occ[0].mean() > 0.02


@pytest.mark.parametrize("kind", ["needles", "slivers"])
def test_rays_in_a_triangle_plane_never_hit_it_and_no_tree_changes_an_answer(rt, orc, builder_options, kind):
    """The hit definition's determinant floor (csrc/rtx_math.hpp: tri_det_floor; oracle tri_hit): for a ray lying in a triangle's plane Moeller-Trumbore is 0 / 0 — without the
    floor float arithmetic accepts u = v = -0 with an arbitrary t there, a hit that brute force reports and a tree finds or not depending on the boxes it visits (the hole
    VERDICT r04 named; tools/soup_lab.cpp measures 7-8 such rays per 600 000 on these soups).  With it: (1) a triangle is never hit by a ray constructed inside its own plane,
    (2) the oracle's brute force, the oracle's own BVH and the host replay of the device traversal on the product's tree — default builder and spatial splits — agree on
    EVERY ray, ids and distances, closest hit and any hit, (3) every reported hit point lies on its triangle (float64)."""
    rng = np.random.default_rng(17 + len(kind))
    n = 3000
    if kind == "needles":
        t = _lab_soup("needles", n, rng)
    else:                                # aspect ratios 10 ... 1e5, lengths 0.01 ... 0.3
        c = rng.uniform(-1, 1, (n, 3)); dd = rng.normal(size=(n, 3)); dd /= np.linalg.norm(dd, axis=1, keepdims=True)
        L = 10.0 ** rng.uniform(-2, -0.5, (n, 1)); w = L * 10.0 ** rng.uniform(-5, -1, (n, 1))
        t = np.stack([c, c + L * dd, c + 0.5 * L * dd + w * rng.normal(size=(n, 3))], axis=1).astype(np.float32)
    m = 30000
    lo, hi = t.reshape(-1, 3).min(0), t.reshape(-1, 3).max(0)
    org = rng.uniform(lo - 0.1, hi + 0.1, (m, 3)); d = rng.normal(size=(m, 3))
    pick = rng.integers(0, n, m // 3); w3 = rng.dirichlet((1, 1, 1), m // 3); w3[: m // 12] = np.eye(3)[rng.integers(0, 3, m // 12)]
    d[: m // 3] = (t[pick] * w3[:, :, None]).sum(1) - org[: m // 3]
    k = m // 3; pl = rng.integers(0, n, k); T = t[pl].astype(np.float64)              # in-plane rays
    a = rng.normal(scale=3.0, size=(k, 2)); b = rng.normal(size=(k, 2))
    org[-k:] = T[:, 0] + a[:, :1] * (T[:, 1] - T[:, 0]) + a[:, 1:] * (T[:, 2] - T[:, 0])
    d[-k:] = b[:, :1] * (T[:, 1] - T[:, 0]) + b[:, 1:] * (T[:, 2] - T[:, 0])
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-30)
    rays = np.zeros((m, 8), np.float32); rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = org, 1e-5, d, 1e30

    class Soup:
        materials = np.zeros((2, 32), np.float32)
        def __init__(self, tris):
            nn = len(tris); v = np.zeros((3 * nn, 7), np.float32); v[:, 0:3] = tris.reshape(-1, 3)
            self.meshes = [(v, np.arange(3 * nn, dtype=np.uint32), np.ones(3 * nn, np.uint32))]
            self.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
        def view_proj(self, aspect):
            e = np.eye(4, dtype=np.float32).reshape(16); return e, e

    o = orc.Oracle().load(Soup(t), 1.0)
    ref = o.trace_closest(rays, mode=0)
    hit = bits(ref)[:, 3] != 0xFFFFFFFF
    assert hit.mean() > 0.1
    assert not (bits(ref)[-k:, 3] == pl).any(), "a ray lying in a triangle's plane hit that triangle"
    P = rays[hit, 0:3].astype(np.float64) + ref[hit, 0:1].astype(np.float64) * rays[hit, 4:7].astype(np.float64)
    tv = t[bits(ref)[hit, 3].astype(np.int64)].astype(np.float64)
    Q = tv[:, 0] + ref[hit, 1:2] * (tv[:, 1] - tv[:, 0]) + ref[hit, 2:3] * (tv[:, 2] - tv[:, 0])
    assert (np.abs(P - Q).max(1) <= 0.02 * float((hi - lo).max())).all(), "a reported hit point lies nowhere near its triangle"
    assert np.array_equal(bits(o.trace_closest(rays, mode=1)), bits(ref)), "the oracle's BVH differs from its brute force"
    sh = rays.copy(); sh[:, 7] = rng.uniform(0.02, 2.0, m).astype(np.float32)
    occ = o.trace_any(sh, mode=0)
    assert np.array_equal(o.trace_any(sh, mode=1), occ)
    for opts in (dict(), dict(split=1e-6, reinsert=3)):
        builder_options(**opts)
        got, refs = rt.bvh_replay(t, rays)
        assert np.array_equal(bits(got)[:, 3], bits(ref)[:, 3]) and np.array_equal(bits(got)[hit, 0], bits(ref)[hit, 0]), opts
        for order in (0, 1, 2):
            assert np.array_equal(bits(rt.bvh_replay(t, sh, any_hit=True, any_order=order)[0])[:, 3] != 0xFFFFFFFF, occ != 0), (opts, order)


def test_anyhit_order_probe_is_deterministic_and_scene_dependent(rt, cornell):
    """probe_anyhit_order (rtx_commit_scene): 2 048 NEE-like segments replayed on the host in the three visiting orders.  Deterministic; the atrium under its sky quad keeps slot
    order, the street with its closed emissive lamp boxes — most NEE segments end on a lamp face that looks away, so the lamp's own housing is the occluder at the FAR end — takes
    farthest-first; a tiny scene (no tree) has nothing to order.  (GPU side: `k_trace_shadow` on the street 9.8 ms in slot order, 8.9 ms farthest first, profiles/r04_pmc_bvh.md)"""
    assert cornell.anyhit_order() == 0
    atrium, street = rt.Scene.sponza_class(60000, 260), rt.Scene.bistro_class(300000, 3800)
    assert atrium.anyhit_order() == 0
    assert street.anyhit_order() == 2
    assert rt.Scene.bistro_class(300000, 3800).anyhit_order() == 2


# ---- the C-ABI library -------------------------------------------------------------------------
def declared_functions(header):
    src = re.sub(r"/\*.*?\*/", "", open(header).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(rtxh?_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol(rt):
    for h in ("rtx.h", "rtx_host.h"):
        names = declared_functions(os.path.join(ROOT, "include", h))
        assert len(names) >= 20
        for n in names:
            assert hasattr(rt.lib, n), f"{n} declared in include/{h} but not exported by librtx_hip.so"


def test_product_library_keeps_the_process_allocator_never_destroys_streams_and_stages_host_copies():
    """Round 5 (profiles/r05_determinism.md): (1) the heap fence that hunted the stray write (csrc/rtx_heap_fence.cpp) is an EMPTY translation unit in the product — librtx_hip.so
    must not define operator new / delete; (2) the cure: the library borrows its HIP streams from a process-wide pool and never destroys one — no call to hipStreamDestroy is
    left in any file of csrc/, nor in host/MultiGpu.cpp (the native N-GPU frame keeps its ranks' streams in a list of its own); (3) every copy between host arrays and the
    device goes through rtx_staging.hpp — in all of csrc/ one direct device-to-host copy remains, the pinned counter block of a path-tracer frame (rtx_render.hip)."""
    pkg = os.path.join(ROOT, "royaltracer-dx_amd")
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(pkg, "librtx_hip.so")], capture_output=True, text=True).stdout
    assert "operator new" not in nm and "operator delete" not in nm
    csrc = sorted(glob.glob(os.path.join(pkg, "csrc", "*")))
    assert len(csrc) >= 20
    for f in csrc + [os.path.join(pkg, "host", "MultiGpu.cpp")]:
        assert "hipStreamDestroy(" not in re.sub(r"//[^\n]*", "", open(f).read()), f
    # host copies go through rtx_staging.hpp; the one left fills the PINNED counter block of a frame
    rest = "".join(open(f).read() for f in csrc if os.path.basename(f) != "rtx_staging.hpp")
    assert "hipMemcpyHostToDevice" not in rest and rest.count("hipMemcpyDeviceToHost") == 1
    assert open(os.path.join(pkg, "csrc", "rtx_render.hip")).read().count("hipMemcpyDeviceToHost") == 1


def test_device_memory_events_and_pinned_memory_are_owned_by_the_owning_types():
    """csrc/rtx_devmem.hpp (and the staging chunks of rtx_staging.hpp) allocate, free and destroy every buffer and event of the library: a resource is a member of an
    owning type and is released by its destructor, with no hand-kept list of buffers to forget one in."""
    pkg = os.path.join(ROOT, "royaltracer-dx_amd")
    others = [f for f in sorted(glob.glob(os.path.join(pkg, "csrc", "*"))) if os.path.basename(f) not in ("rtx_devmem.hpp", "rtx_staging.hpp")]
    assert len(others) >= 20
    for f in others:
        src = re.sub(r"//[^\n]*", "", open(f).read())
        for call in ("hipMalloc(", "hipFree(", "hipHostMalloc(", "hipHostFree(", "hipEventDestroy("):
            assert call not in src, (f, call)


def test_kernels_live_in_headers_by_concern_and_the_chunk_deal_is_written_once():
    """csrc/rtx_kernels.hip is the map of the design, the kernel headers' one translation unit and their launchers: it defines no kernel itself.  Every launcher declared in
    rtx_kernels.hpp is defined exactly once across the .hip files (the refit and tree-cost launchers in rtx_refit.hip).  The chunk deal of the raygen kernels (rows rotated by
    k * 2654435761u % nk) is written in ONE place, dealt_chunk in rtx_dev_common.hpp — and once more inside k_raygen_trace_small, which keeps it written out because the compiler
    allocates that kernel's registers differently through the helper (profiles/kernels_split_isa.md); no third copy."""
    csrc = os.path.join(ROOT, "royaltracer-dx_amd", "csrc")
    assert "__global__" not in open(os.path.join(csrc, "rtx_kernels.hip")).read()
    declared = re.findall(r"^void (launch_\w+)\(", open(os.path.join(csrc, "rtx_kernels.hpp")).read(), re.M)
    assert len(declared) >= 40 and len(set(declared)) == len(declared)
    hips = {f: open(f).read() for f in sorted(glob.glob(os.path.join(csrc, "*.hip")))}
    assert len(hips) >= 8
    for name in declared:
        where = [os.path.basename(f) for f, src in hips.items() for _ in re.findall(r"^void %s\(" % name, src, re.M)]
        assert len(where) == 1, (name, where)
    deal = re.compile(r"2654435761u\)\s*%\s*nk\b")
    copies = {os.path.basename(f): len(deal.findall(open(f).read())) for f in sorted(glob.glob(os.path.join(csrc, "*")))}
    assert {f: n for f, n in copies.items() if n} == {"rtx_dev_common.hpp": 1, "rtx_k_raygen.hpp": 1}
    raygen = open(os.path.join(csrc, "rtx_k_raygen.hpp")).read()
    kept = raygen[raygen.index("void k_raygen_trace_small("):raygen.index("void k_primary_surface(")]
    assert len(deal.findall(kept)) == 1 and "dealt_chunk" in kept           # the written-out copy names the helper it must equal


def test_no_cpu_fallback_without_a_gpu(rt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(rt.RtxError) as e:
        rt.Context(0)
    assert "no HIP device" in str(e.value) or "no CPU fallback" in str(e.value)


def test_product_never_references_the_oracle():
    pkg = os.path.join(ROOT, "royaltracer-dx_amd")
    for dp, _, files in os.walk(pkg):
        if os.path.basename(dp) == "build":
            continue
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".hpp", ".h")) or f == "Makefile":
                txt = open(os.path.join(dp, f), errors="ignore").read()
                # comments may mention the oracle; including, importing, linking or loading it is forbidden
                for pat in (r"#\s*include[^\n]*oracle", r"\bimport\s+orc\b", r"\bfrom\s+oracle\b", r"librt_oracle", r"-lrt_oracle", r"rt_oracle\.h", r"orc_[a-z_]+\s*\("):
                    assert not re.search(pat, txt), (os.path.join(dp, f), pat)
    ldd = subprocess.run(["ldd", os.path.join(pkg, "librtx_hip.so")], capture_output=True, text=True).stdout
    assert "oracle" not in ldd and "amdhip64" in ldd


def test_params_struct_layout(rt, orc):
    assert ctypes.sizeof(rt.Params) == ctypes.sizeof(orc.Params) == 48
    assert [n for n, _ in rt.Params._fields_] == [n for n, _ in orc.Params._fields_]


def test_tiny_scene_pretest_records_are_conservative(rt, orc, cornell):
    """The plane/edge pre-test of the tiny-scene path (rtx_small_scene.cpp) may only discard triangles the exact test
    rejects: emulate it in float64 for every brute-force hit of 100 k rays (camera, random, from-surface, grazing)."""
    recs, ids, delta, cm = cornell.small_records()
    assert len(recs) == 17 and (ids[:, 1] >= 0).sum() == 15                    # 15 planar quads + 2 single triangles (the twisted red wall)
    assert sorted(int(v) for v in ids.ravel() if v >= 0) == list(range(32))    # every triangle in exactly one record
    o = orc.Oracle().load(cornell, 16 / 9)
    rng = np.random.default_rng(3)
    n = 60000
    r = np.zeros((n, 8), np.float32); r[:, 0:3] = rng.uniform(-0.2, 1.2, (n, 3)); d = rng.normal(size=(n, 3)); r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3], r[:, 7] = 1e-4, 1e4
    cam = o.primary_rays(rt.Params(width=160, height=90)); hc = o.trace_closest(cam, 1); hitc = hc.view(np.uint32)[:, 3] != 0xFFFFFFFF
    sec = np.zeros((int(hitc.sum()), 8), np.float32); sec[:, 0:3] = cam[hitc, 0:3] + hc[hitc, 0:1] * cam[hitc, 4:7]
    d = rng.normal(size=(len(sec), 3)); sec[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True); sec[:, 3], sec[:, 7] = 2e-5, 1e4
    graz = r[:8000].copy(); graz[:, 5] = rng.uniform(-2e-4, 2e-4, len(graz)); graz[:, 4:7] /= np.linalg.norm(graz[:, 4:7], axis=1, keepdims=True)
    rays = np.concatenate([cam, r, sec, graz])
    h = o.trace_closest(rays, 0); prim = h.view(np.uint32)[:, 3]; hit = prim != 0xFFFFFFFF
    owner = np.full(32, -1); owner[ids[:, 0]] = np.arange(len(ids)); two = ids[:, 1] >= 0; owner[ids[two, 1]] = np.arange(len(ids))[two]
    R = recs.astype(np.float64)[owner[prim[hit]]]
    oo, dd = rays[hit, 0:3].astype(np.float64), rays[hit, 4:7].astype(np.float64)
    nd = (R[:, 0:3] * dd).sum(1); no = R[:, 3] - (R[:, 0:3] * oo).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = no / nd
        P = oo + t[:, None] * dd
        e = np.stack([(R[:, 4 + 4 * j:7 + 4 * j] * P).sum(1) + R[:, 7 + 4 * j] for j in range(4)], 1)
        mt = cm * np.abs(1 / nd) + 1e-5 * np.abs(t)
        tmin, tmax = rays[hit, 3].astype(np.float64), rays[hit, 7].astype(np.float64)
        ok = (t + mt >= tmin) & (tmax + mt - t >= 0) & (e.min(1) + delta >= 0)
    passes = ok | (np.abs(nd) < 1e-3)
    assert passes.all(), f"{int((~passes).sum())} true hits would be discarded by the pre-test"
    assert hit.sum() > 40000


def test_bvh_refit_keeps_invariants(rt):
    rng = np.random.default_rng(12)
    n = 3000
    c = rng.uniform(-1, 1, (n, 1, 3)); a = (c + rng.normal(scale=0.03, size=(n, 3, 3))).astype(np.float32)
    ang = 0.7; R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]], np.float32)
    b = a.copy(); b[: n // 2] = b[: n // 2] @ R.T + np.float32([0.3, -0.2, 0.1])      # half of the triangles move rigidly
    assert rt.bvh_refit_check(a.reshape(-1, 9), b.reshape(-1, 9)) == 0
    assert rt.bvh_refit_check(a.reshape(-1, 9), a.reshape(-1, 9)) == 0


# ---- image writers (headless display path) ------------------------------------------------------
def test_png_ppm_exr_writers_round_trip(rt, tmp_path):
    import struct, zlib
    rng = np.random.default_rng(3)
    W, H = 37, 21
    img = rng.integers(0, 256, (H, W, 4), dtype=np.uint8)
    # PNG: signature, chunk CRCs, IHDR fields, and the inflated scanlines equal the input
    p = str(tmp_path / "a.png"); rt.write_image(p, img)
    b = open(p, "rb").read()
    assert b[:8] == b"\x89PNG\r\n\x1a\n"
    at, chunks = 8, []
    while at < len(b):
        n, typ = struct.unpack(">I4s", b[at:at + 8]); data = b[at + 8:at + 8 + n]; crc, = struct.unpack(">I", b[at + 8 + n:at + 12 + n])
        assert zlib.crc32(typ + data) == crc
        chunks.append((typ, data)); at += 12 + n
    assert [c[0] for c in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert struct.unpack(">IIBBBBB", chunks[0][1]) == (W, H, 8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8).reshape(H, 1 + W * 4)
    assert (raw[:, 0] == 0).all() and np.array_equal(raw[:, 1:].reshape(H, W, 4), img)
    # a frame larger than one stored deflate block (65535 bytes)
    big = rng.integers(0, 256, (200, 300, 4), dtype=np.uint8)
    p2 = str(tmp_path / "b.png"); rt.write_image(p2, big)
    b2 = open(p2, "rb").read(); i = b2.index(b"IDAT"); n, = struct.unpack(">I", b2[i - 4:i])
    assert np.array_equal(np.frombuffer(zlib.decompress(b2[i + 4:i + 4 + n]), np.uint8).reshape(200, 1 + 1200)[:, 1:].reshape(200, 300, 4), big)
    # PPM
    p = str(tmp_path / "a.ppm"); rt.write_image(p, img)
    b = open(p, "rb").read(); hdr = b"P6\n%d %d\n255\n" % (W, H)
    assert b.startswith(hdr) and np.array_equal(np.frombuffer(b[len(hdr):], np.uint8).reshape(H, W, 3), img[..., :3])
    # EXR: header attributes, offset table, scanlines hold accum.xyz / count as B, G, R planes
    acc = rng.uniform(0, 4, (H, W, 4)).astype(np.float32); acc[..., 3] = rng.integers(0, 5, (H, W))
    p = str(tmp_path / "a.exr"); rt.write_image(p, acc)
    b = open(p, "rb").read()
    assert struct.unpack("<II", b[:8]) == (20000630, 2)
    at, attrs = 8, {}
    while b[at] != 0:
        e = b.index(b"\0", at); name = b[at:e].decode(); at = e + 1
        e = b.index(b"\0", at); typ = b[at:e].decode(); at = e + 1
        n, = struct.unpack("<I", b[at:at + 4]); attrs[name] = (typ, b[at + 4:at + 4 + n]); at += 4 + n
    at += 1
    assert attrs["compression"] == ("compression", b"\0") and attrs["lineOrder"] == ("lineOrder", b"\0")
    assert struct.unpack("<4i", attrs["dataWindow"][1]) == (0, 0, W - 1, H - 1) and attrs["dataWindow"] == attrs["displayWindow"]
    ch = attrs["channels"][1]; names = []
    k = 0
    while ch[k] != 0:
        e = ch.index(b"\0", k); names.append(ch[k:e].decode()); assert struct.unpack("<I", ch[e + 1:e + 5]) == (2,); k = e + 17
    assert names == ["B", "G", "R"]
    offs = struct.unpack("<%dQ" % H, b[at:at + 8 * H])
    want = acc[..., :3] / np.maximum(acc[..., 3:4], 1.0)
    for y in (0, H // 2, H - 1):
        yy, nb = struct.unpack("<iI", b[offs[y]:offs[y] + 8]); assert (yy, nb) == (y, W * 12)
        line = np.frombuffer(b[offs[y] + 8:offs[y] + 8 + nb], np.float32).reshape(3, W)
        assert np.array_equal(line[0], want[y, :, 2]) and np.array_equal(line[1], want[y, :, 1]) and np.array_equal(line[2], want[y, :, 0])
    assert len(b) == offs[-1] + 8 + W * 12
    with pytest.raises(rt.RtxError):
        rt.write_image(str(tmp_path / "no_such_dir" / "x.png"), img)


def test_tiny_scene_hull_faces_come_last(rt, cornell):
    """NEE shadow segments skip the records behind small_occluders(): those must be exactly the records whose plane has every
    scene vertex on one side (faces of the convex hull: the five walls of the Cornell Box), checked here in float64"""
    recs, ids, delta, cm = cornell.small_records()
    nocc = cornell.small_occluders()
    v, idx, _ = cornell.meshes[0]
    P = v[:, :3].astype(np.float64)
    side = recs[:, 0:3].astype(np.float64) @ P.T - recs[:, 3:4].astype(np.float64)          # (records, vertices): signed distance to the plane
    both = ((side > 1e-6).any(1)) & ((side < -1e-6).any(1))
    assert nocc == 11 and len(recs) == 17                 # 6 hull records: floor, ceiling, back, green wall, and the twisted red wall as 2 single triangles
    assert both[:nocc].all() and not both[nocc:].any()
    # the hull faces are the floor, ceiling, back, left and right walls: together they own 10 triangles
    assert (ids[nocc:] >= 0).sum() == 10


def _host_layer_sources(pk):
    """the C++ host layer without the device API: the host scene and its BVH, the scene cache, the host facade (what the sanitizer runs compile beside their driver)"""
    csrc = ("rtx_scene_host.cpp", "rtx_small_scene.cpp", "rtx_bvh_build.cpp", "rtx_bvh_wide.cpp", "rtx_bvh_replay.cpp", "rtx_scene_cache.cpp")
    host = ("DirectXMathLite.cpp", "manipulator.cpp", "ObjLoader.cpp", "Scenes.cpp", "Renderer.cpp", "ImageIO.cpp", "rtx_host_c.cpp")
    return [os.path.join(pk, "csrc", f) for f in csrc] + [os.path.join(pk, "host", f) for f in host]


def test_host_layer_under_asan_ubsan(tmp_path, golden_dir):
    """the C++ host layer (scene generators, OBJ loader, BVH build / DP collapse / refit / validators, tiny-scene records, image
    writers) compiled with g++ -fsanitize=address,undefined and run on the CPU with the device API stubbed"""
    import subprocess, shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pk = os.path.join(root, "royaltracer-dx_amd")
    srcs = [os.path.join(root, "tests", "sanitize", f) for f in ("host_main.cpp", "device_stubs.cpp")] + _host_layer_sources(pk)
    exe = str(tmp_path / "san_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(pk, "csrc"), "-I" + os.path.join(pk, "host"), "-pthread", "-o", exe] + srcs
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe, golden_dir, str(tmp_path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "done" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_map_slot_table_under_asan_ubsan(tmp_path):
    """the host scene's map-slot table as a stand-alone program (tests/sanitize/mapslots_main.cpp, its own main) compiled with g++ -fsanitize=address,undefined and run
    as a child process: every slot on a plain, an emitting and an unused material against the rules of include/rtx.h, written out by hand in the driver"""
    import subprocess, shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pk = os.path.join(root, "royaltracer-dx_amd")
    srcs = [os.path.join(root, "tests", "sanitize", f) for f in ("mapslots_main.cpp", "device_stubs.cpp")] + _host_layer_sources(pk)
    exe = str(tmp_path / "san_mapslots")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(pk, "csrc"), "-I" + os.path.join(pk, "host"), "-pthread", "-o", exe] + srcs
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "done" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]


def test_parallel_builder_under_tsan(tmp_path):
    """"same tree for any thread count" is a correctness premise of the parallel top-down build, so the threaded host code runs under ThreadSanitizer
    (g++ -fsanitize=thread, CPU only, device API stubbed): build + re-insertion + wide collapse with 1 / 3 / 16 builder threads on 66 000 triangles — the three trees replay
    the same traversal ray for ray —, and a whole scene build with the commit-time any-hit probe.  No data race may be reported."""
    import subprocess, shutil
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pk = os.path.join(root, "royaltracer-dx_amd")
    srcs = [os.path.join(root, "tests", "sanitize", f) for f in ("tsan_main.cpp", "device_stubs.cpp")] + _host_layer_sources(pk)
    exe = str(tmp_path / "tsan_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(root, "include"), "-I" + os.path.join(pk, "csrc"), "-I" + os.path.join(pk, "host"), "-pthread", "-o", exe] + srcs
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if b.returncode != 0 and "tsan" in b.stderr.lower() and "cannot find" in b.stderr.lower():
        pytest.skip("libtsan not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900, env=dict(os.environ, TSAN_OPTIONS="halt_on_error=0:second_deadlock_stack=1"), cwd=str(tmp_path))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "done" in r.stdout and "ThreadSanitizer" not in r.stderr and "data race" not in r.stderr, r.stderr[-3000:]


def test_scene_cache_round_trip_and_rejects_damaged_files(rt, cornell, tmp_path, golden_dir):
    """SURVEY 8(f3) binary scene cache on the host (no GPU): save -> load gives back the same materials, meshes, instances and camera;
    a truncated file, a flipped payload byte, a foreign file and another version are all refused with a message and nothing loaded."""
    import os
    for name, sc in (("cornell", cornell), ("garage", rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")),
                     ("atrium", rt.Scene.sponza_class(20000, 260))):
        path = tmp_path / (name + ".rtxscn")
        sc.save(path)
        back = rt.Scene.load(path)
        assert np.array_equal(back.materials.view(np.uint32), sc.materials.view(np.uint32))
        assert len(back.meshes) == len(sc.meshes) and len(back.instances) == len(sc.instances) and back.num_triangles == sc.num_triangles
        for (v0, i0, m0), (v1, i1, m1) in zip(sc.meshes, back.meshes):
            assert np.array_equal(v0.view(np.uint32), v1.view(np.uint32)) and np.array_equal(i0, i1) and np.array_equal(m0, m1)
        for (a, ma), (b, mb) in zip(sc.instances, back.instances):
            assert a == b and np.array_equal(ma, mb)
        assert np.array_equal(back.eye, sc.eye) and np.array_equal(back.center, sc.center) and back.fovy_deg == sc.fovy_deg
        for x, y in zip(back.view_proj(1.5), sc.view_proj(1.5)):
            assert np.array_equal(x, y)
    blob = bytearray(open(path, "rb").read())
    assert blob[:8] == b"RTXSCN01" and len(blob) > 1 << 20

    def refused(data, what):
        bad = tmp_path / "bad.rtxscn"
        bad.write_bytes(bytes(data))
        with pytest.raises(rt.RtxError) as e:
            rt.Scene.load(bad)
        assert what in str(e.value), str(e.value)
    refused(blob[:len(blob) // 2], "length")
    flipped = bytearray(blob); flipped[len(blob) // 2] ^= 0x10
    refused(flipped, "checksum")
    refused(b"P6\n" + bytes(200), "not a scene cache")
    newer = bytearray(blob); newer[8] = 9
    refused(newer, "version")
    with pytest.raises(rt.RtxError):
        rt.Scene.load(tmp_path / "missing.rtxscn")

    # CRAFTED files: the checksum is a word hash, not a signature, so a file that carries a valid one must still be refused when a field the kernels
    # or the refit trust is out of range (mesh count, traversal stack depth, vertex indices, instance triangle ranges).  The hash of
    # csrc/rtx_scene_cache.cpp restated here (4 lanes over 64-bit words per 4 MiB chunk, chunks folded in order).
    M64 = (1 << 64) - 1

    def mix(h, w):
        h = ((h ^ w) * 0x9E3779B97F4A7C15) & M64
        return h ^ (h >> 29)

    def hash_chunk(b):
        h = [0x243F6A8885A308D3, 0x13198A2E03707344, 0xA4093822299F31D0, 0x082EFA98EC4E6C89]
        n = len(b); full = n - n % 32
        w = np.frombuffer(bytes(b[:full]), dtype="<u8").tolist()
        for i in range(0, len(w), 4):
            for k in range(4):
                h[k] = mix(h[k], w[i + k])
        tail = np.frombuffer(bytes(b[full:]) + bytes(32 - (n - full)), dtype="<u8").tolist()
        for k in range(4):
            h[k] = mix(h[k], tail[k])
        return mix(mix(mix(mix(n, h[0]), h[1]), h[2]), h[3])

    def resign(data):
        pay = data[80:]
        h = 0x452821E638D01377 ^ len(pay)
        for c in range(0, len(pay), 4 << 20):
            h = mix(h, hash_chunk(pay[c:c + (4 << 20)]))
        data[56:64] = int(h).to_bytes(8, "little")            # Header: magic 8, version 4, endian 4, layout 32, payload 8, checksum 8, sections 8
        return data

    small = tmp_path / "cornell.rtxscn"
    blob = bytearray(open(small, "rb").read())
    assert bytes(resign(bytearray(blob))) == bytes(blob)                            # the restated hash reproduces the file's own checksum
    rt.Scene.load(small)
    # the scalar block follows the first section head: payload offset 16; Scalars = {stack8, small_nrec, small_nocc, max_depth, nmesh, ...}
    sc0 = 80 + 16
    def patched(off, value):
        d = bytearray(blob); d[off:off + 4] = int(value).to_bytes(4, "little"); return resign(d)
    refused(patched(sc0 + 16, 0x7FFFFFFF), "mesh count")                           # nmesh: used to size a vector
    refused(patched(sc0 + 16, 3), "unexpected section")                            # nmesh: more meshes than sections
    refused(patched(sc0 + 0, 7), "stack depth")                                    # stack8: sizes the per-lane LDS stack column
    refused(patched(sc0 + 4, 65), "inconsistent")                                  # small_nrec beyond the tiny-scene limit / the stored records
    # a vertex index beyond the mesh's vertices: find the first T_MESHI section (tag 6, element size 4) and poison its first entry
    at, tag_meshi = 80, 6
    while at < len(blob):
        tag, elem = int.from_bytes(blob[at:at + 4], "little"), int.from_bytes(blob[at + 4:at + 8], "little")
        cnt = int.from_bytes(blob[at + 8:at + 16], "little")
        if tag == tag_meshi:
            break
        at += 16 + ((elem * cnt + 15) & ~15)
    assert tag == tag_meshi and elem == 4 and cnt >= 3
    refused(patched(at + 16, 0x00FFFFFF), "inconsistent")
    # InstHost::tri_base (the last dword of the 264-byte record; section tag 4)
    at = 80
    while True:
        tag, elem = int.from_bytes(blob[at:at + 4], "little"), int.from_bytes(blob[at + 4:at + 8], "little")
        cnt = int.from_bytes(blob[at + 8:at + 16], "little")
        if tag == 4:
            break
        at += 16 + ((elem * cnt + 15) & ~15)
    assert elem == 264 and cnt >= 1
    refused(patched(at + 16 + 260, 5), "inconsistent")


def test_scene_cache_keeps_material_extension_records_and_texture_names(rt, golden_dir, tmp_path):
    """an OBJ / MTL scene that goes through Scene.save() / Scene.load() answers the MaterialExt / texture accessors as before
    (the cache carries both beside the material table: format version 2)."""
    D = os.path.join(golden_dir, "mtlext")
    sc = rt.Scene.from_obj([os.path.join(D, "mx03.obj")], D + "/")
    assert sc.material_ext and sc.textures
    path = tmp_path / "mx03.rtxscn"
    sc.save(path)
    back = rt.Scene.load(path)
    assert back.textures == sc.textures and back.material_ext == sc.material_ext
    cb = rt.Scene.cornell(); cb.save(tmp_path / "c.rtxscn")
    assert rt.Scene.load(tmp_path / "c.rtxscn").material_ext == []


def test_mtl_extension_keys_and_map_ids_match_tinyobj(rt, golden_dir):
    """every MTL statement the reference's vendored tinyobjloader v2.0.0 reads — Ka Kd Ks Ke Tf/Kt Ns Ni d illum, the PBR
    extension Pr Pm Ps Pc Pcr aniso anisor, and all map_* / bump / disp / refl / norm statements with their options — parsed by our reader
    and compared with what tinyobj parsed from the same 10 random files (tests/golden/mtlext, make_mtl_ext.py).  The 128-byte Material
    takes what the reference copies into it (ObjLoader.h:428-435); the rest rides beside it as MaterialExt + texture ids."""
    D = os.path.join(golden_dir, "mtlext")
    ref = json.load(open(os.path.join(D, "ref.json")))
    f32 = lambda v: np.asarray(v, np.float32)
    ntex = 0
    for k in range(10):
        sc = rt.Scene.from_obj([os.path.join(D, "mx%02d.obj" % k)], D + "/")
        mats = ref["mx%02d" % k]
        assert len(sc.materials) == 1 + len(mats) == len(sc.material_ext)
        d = sc.material_ext[0]                                                            # the default material's record: tinyobj's initial values
        assert (d["Ni"], d["Ns"], d["Pcr"], d["aniso"], d["anisor"], d["illum"], d["maps"]) == (1.0, 1.0, 0.0, 0.0, 0.0, 0, {})
        for j, m in enumerate(mats):
            g, x = sc.materials[1 + j], sc.material_ext[1 + j]
            assert np.array_equal(bits(g[0:3]), bits(f32(m["diffuse"]))) and bits(g[3:4])[0] == bits(f32([m["dissolve"]]))[0], (k, j)
            assert np.array_equal(bits(g[4:7]), bits(f32(m["specular"]))) and np.array_equal(bits(g[8:11]), bits(f32(m["emission"]))), (k, j)
            assert np.array_equal(bits(g[12:16]), bits(f32([m["roughness"], m["metallic"], m["sheen"], m["clearcoat_thickness"]]))), (k, j)
            assert g[7] == 1.0                                                            # Material.Ni is never filled by the reference's loader
            got = f32([x["Ni"], x["Ns"], x["Pcr"], x["aniso"], x["anisor"]] + x["Ka"] + x["Tf"])
            exp = f32([m["ior"], m["shininess"], m["clearcoat_roughness"], m["anisotropy"], m["anisotropy_rotation"]] + m["ambient"] + m["transmittance"])
            assert np.array_equal(bits(got), bits(exp)) and x["illum"] == m["illum"], (k, j, got, exp)
            exp_maps = {rt.MAP_SLOTS[s]: t for s, t in enumerate(m["tex"]) if t}
            assert x["maps"] == exp_maps, (k, j, x["maps"], exp_maps)
            ntex += len(exp_maps)
        assert sorted(sc.textures) == sorted({t for m in mats for t in m["tex"] if t})      # one id per distinct file name
    assert ntex > 80 and any(" " in t for t in sc.textures + [t for v in ref.values() for m in v for t in m["tex"]])   # names with blanks occur
    assert rt.Scene.cornell().material_ext == []                                           # synthetic scenes carry none


def test_bench_asset_policy_loads_real_models_when_present(rt, golden_dir, tmp_path, monkeypatch):
    """SURVEY 8(d) / BASELINE.md: "assets/sponza.obj / assets/bistro.obj loaded if present, else procedural" (the reference loads its models in Renderer.cpp:363-370 through
    ObjLoader::loadObjFile).  bench.make_scene looks under $RTX_ASSETS and <repo>/assets; tests/golden/garage.obj stands in for the asset here: it is picked up, named in the
    scene description with its triangle count, and framed by a camera inside its bounding box; without a file the procedural scene of the class is used."""
    import importlib, shutil, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    bench = importlib.import_module("bench")
    monkeypatch.setenv("RTX_ASSETS", str(tmp_path))
    if not os.path.isfile(os.path.join(root, "assets", "sponza.obj")):
        assert bench.asset_path("sponza") is None
    shutil.copy(os.path.join(golden_dir, "garage.obj"), tmp_path / "sponza.obj")
    shutil.copy(os.path.join(golden_dir, "garage.mtl"), tmp_path / "garage.mtl")
    sc, source = bench.make_scene(rt, "sponza")
    assert source.startswith("asset:") and "sponza.obj" in source and "1254 triangles" in source and sc.num_triangles == 1254
    assert len(sc.materials) == 4 and sc.materials[3][8:11].sum() > 0            # the MTL was found beside the OBJ: default + 3 materials, `lights` is emissive
    lo, hi = sc.bounds()
    assert (sc.eye > lo - 1e-3).all() and (sc.eye < hi + 1e-3).all()             # the camera sits inside the model
    v, p = sc.view_proj(16 / 9)
    assert np.isfinite(v).all() and np.isfinite(p).all()
    if not os.path.isfile(os.path.join(root, "assets", "bistro.obj")):
        assert bench.asset_path("bistro") is None                                # nothing there: bench falls back to the generator (not built here: 3.8 M triangles)


def test_bench_dump_outputs_samples_an_image_above_its_limit(tmp_path):
    """bench.py --dump-outputs: an image up to DUMP_IMAGE_BYTES is written whole as accum.npy; a larger one (a 3840 x 2160 frame) as a fixed, seeded pixel sample,
    accum_sample.npy, the same pixels on every run, taken from the image unchanged; with rays.npy the whole dump stays within 64 MB"""
    import importlib, sys
    sys.path.insert(0, ROOT)
    bench = importlib.import_module("bench")
    rays = [8294400, 1.5e9, 1.2e9]
    small = np.random.default_rng(1).random((54, 96, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "small"), small, rays)
    assert sorted(os.listdir(tmp_path / "small")) == ["accum.npy", "rays.npy"]
    assert np.array_equal(bits(np.load(tmp_path / "small" / "accum.npy")), bits(small))
    pix = np.arange(2160 * 3840)
    big = np.stack([pix // 4096, pix % 4096, pix % 7, pix % 11], axis=-1).astype(np.float32).reshape(2160, 3840, 4)   # channels 0 / 1 name the pixel exactly
    assert big.nbytes > bench.DUMP_IMAGE_BYTES
    dumps = []
    for run in ("a", "b"):
        d = tmp_path / run
        bench.dump_outputs(str(d), big, rays)
        assert sorted(os.listdir(d)) == ["accum_sample.npy", "rays.npy"]
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= 64 << 20
        dumps.append(np.load(d / "accum_sample.npy"))
    s = dumps[0]
    assert s.dtype == np.float32 and s.ndim == 2 and s.shape[1] == 4 and s.nbytes == bench.DUMP_IMAGE_BYTES
    assert np.array_equal(bits(s), bits(dumps[1]))                                         # seeded: the same sample every run
    idx = s[:, 0].astype(np.int64) * 4096 + s[:, 1].astype(np.int64)                      # pixel index of each row
    assert np.array_equal(s, big.reshape(-1, 4)[idx]) and (np.diff(idx) > 0).all()         # pixels of the image, unchanged, distinct, in image order
    assert idx[-1] - idx[0] > 0.9 * 2160 * 3840                                           # spread over the whole frame
    r = np.load(tmp_path / "a" / "rays.npy")
    assert r.dtype == np.float64 and list(r) == rays

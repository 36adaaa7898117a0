"""Emission maps without a GPU: the numpy twin (tests/emimap_ref.py) against hand-computed values on a 2 x 2 and a 5 x 3 texture; the mean of a constant texture; the host
builder's light list — SceneHost::build_lights as a stand-alone program (tests/sanitize/emimap_main.cpp) under the sanitizers — against the twin bit for bit; the MTL
loader's binding of map_Ke with its unit-Ke rule; and the new symbols."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import emimap_ref as em
import texture_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EYE = np.eye(4, dtype=np.float32).reshape(16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the twin against hand-computed values
# ------------------------------------------------------------------------------------------------
def test_split_edge_cases():
    # 2 x 2: an edge of half the texture is one texel — n = 1 exactly at the boundary, 2 just above it
    assert em.split([(0.25, 0.75), (0.75, 0.75), (0.25, 0.25)], 2, 2) == 1
    assert em.split([(0.25, 0.75), (0.76, 0.75), (0.25, 0.25)], 2, 2) == 2
    assert em.split([(0.5, 0.5)] * 3, 2, 2) == 1                               # a degenerate UV triangle: clamped up to 1
    # 5 x 3, not square: the u extent counts 5 texels per unit, the v extent 3; the third edge (corner 2 back to corner 0) counts too
    assert em.split([(0, 0), (1, 0), (0, 1)], 5, 3) == 5 and em.split([(0, 0), (0.1, 1), (0, 0)], 5, 3) == 3
    assert em.split([(0, 0), (0, 0), (2.05, 0)], 5, 3) == 11                   # ceil(10.25)
    assert em.split([(-0.7, -0.7), (1.8, -0.7), (-0.7, 1.8)], 5, 3) == 13      # the wrap: 2.5 x 5 = 12.5
    assert em.split([(0, 0), (3.2, 0), (0, 3.2)], 5, 3) == 16 and em.split([(0, 0), (3.3, 0), (0, 40)], 5, 3) == 16      # the clamp


def test_centroids_order_and_count():
    assert em.centroids(1).tolist() == [[1 / 3, 1 / 3]]
    c = em.centroids(2)
    want = [((0 + 1 / 3) / 2, (0 + 1 / 3) / 2), ((0 + 2 / 3) / 2, (0 + 2 / 3) / 2), ((0 + 1 / 3) / 2, (1 + 1 / 3) / 2), ((1 + 1 / 3) / 2, (0 + 1 / 3) / 2)]
    assert c.tolist() == [list(x) for x in want]                              # i outer, j inner, the upright one of a cell before its inverted one
    for n in (3, 7, 16):
        c = em.centroids(n)
        assert len(c) == n * n and (c > 0).all() and (c.sum(axis=1) < 1).all()
        assert abs(c.mean(axis=0) - 1 / 3).max() < 1e-12                      # equal sub-triangles: their centroids average to the triangle's


def test_mean_on_a_2x2_texture_by_hand():
    px = np.zeros((2, 2, 4), np.uint8); px[0, 0] = (255, 51, 0, 9)            # the top-left texel: 1.0, 0.2, 0; everything else black
    # n = 1, all three corners at one texel centre: s = 0.25, t = 0.75 -> x = 0, y = 0: texel (0, 0) itself
    m = em.triangle_mean(px, False, [(0.25, 0.75)] * 3)
    assert np.array_equal(bits(m), bits([1.0, F(51) / F(255), 0.0]))
    # n = 1, a non-degenerate triangle: the centroid (u, v) = (1/3, 1/3) -> s = 0.25 + 0.5 / 3, t = 0.75 - 0.5 / 3 -> x = y = 1/3: weights (2/3)^2 on texel (0, 0)
    m = em.triangle_mean(px, False, [(0.25, 0.75), (0.75, 0.75), (0.25, 0.25)])
    assert np.allclose(m, [4 / 9, 0.2 * 4 / 9, 0.0], rtol=0, atol=1e-6)
    # the wrap: the same triangle one period to the left and one up
    m2 = em.triangle_mean(px, False, [(0.25 - 1, 0.75 + 1), (0.75 - 1, 0.75 + 1), (0.25 - 1, 0.25 + 1)])
    assert np.allclose(m2, m, rtol=0, atol=1e-6)
    # ... and across the seam: the texel's left neighbour is the LAST column
    px2 = np.zeros((2, 2, 4), np.uint8); px2[0, 1] = 255
    m = em.triangle_mean(px2, False, [(0.125, 0.75)] * 3)                    # x = -0.25: taps (-1 -> 1, 0), weight 0.25 on the last column
    assert np.allclose(m, [0.25] * 3, rtol=0, atol=1e-7)
    # sRGB is honoured
    m = em.triangle_mean(px, True, [(0.25, 0.75)] * 3)
    assert np.array_equal(bits(m), bits([tr.table(True)[255], tr.table(True)[51], 0.0]))


def test_mean_on_a_5x3_texture_by_hand():
    # columns 0 .. 4 hold 0, 50, 100, 150, 200 in red; the rows are equal.  Over u in [0.1, 0.9] (texel centres: the interpolation is linear in u there) the mean of a
    # linear function over a triangle is its value at the centroid, and every sub-triangle centroid sees a linear function: mean = f(centroid of the triangle)
    px = np.zeros((3, 5, 4), np.uint8); px[..., 0] = np.arange(5)[None, :] * 50
    uv = [(0.1, 0.2), (0.9, 0.2), (0.1, 0.8)]
    assert em.split(uv, 5, 3) == 4
    m = em.triangle_mean(px, False, uv)
    s_c = 0.1 + 0.8 / 3                                                        # the centroid's s -> x = 5 s - 0.5
    assert abs(float(m[0]) - (5 * s_c - 0.5) * 50 / 255) < 1e-6 and m[1] == 0 and m[2] == 0
    # n = 16 over several periods of a texture that is not a power of two in either direction: the mean stays inside the texel range and the quadrature is deterministic
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    uv = [(-0.7, -0.7), (2.6, -0.7), (-0.7, 2.6)]
    assert em.split(uv, 5, 3) == 16
    m = em.triangle_mean(px, False, uv)
    lo, hi = px[..., :3].reshape(-1, 3).min(axis=0) / 255.0, px[..., :3].reshape(-1, 3).max(axis=0) / 255.0
    assert (m >= lo - 1e-6).all() and (m <= hi + 1e-6).all() and np.array_equal(bits(m), bits(em.triangle_mean(px, False, uv)))
    assert abs(m - px[..., :3].reshape(-1, 3).mean(axis=0) / 255.0).max() < 0.08     # 3.3 periods each way: near the texture's own mean


def test_mean_of_a_constant_texture_is_the_constant_to_the_bit():
    rng = np.random.default_rng(4)
    for srgb in (False, True):
        for shape, val in (((2, 2), (137, 1, 255)), ((3, 5), (255, 255, 255)), ((3, 5), (7, 200, 33))):
            px = np.zeros(shape + (4,), np.uint8); px[..., :3] = val; px[..., 3] = rng.integers(0, 256, shape)
            T = tr.table(srgb)
            for _ in range(12):
                uv = rng.uniform(-2, 3, (3, 2)).astype(np.float32) * F(rng.choice([0.05, 0.3, 1.0]))
                m = em.triangle_mean(px, srgb, uv)
                assert np.array_equal(bits(m), bits(T[list(val)])), (srgb, shape, val, em.split(uv, shape[1], shape[0]))


def test_weight_terms(rt):
    E, inten, q = em.triangle_weight_terms(rt.half_round, [10.0, 5.0, 2.5], [1.0, 1.0, 1.0])
    assert E.tolist() == [10.0, 5.0, 2.5] and inten == F(17.5) / F(3.0) and q == F(17.5) / F(3.0)
    E, inten, q = em.triangle_weight_terms(rt.half_round, [3.0, 3.0, 3.0], [F(1) / F(3), 0.0, 1.0])
    assert inten == ((F(3.0) * (F(1) / F(3)) + F(0)) + F(3)) / F(3.0)
    assert q == ((F(rt.half_round(float(E[0]))) + F(0)) + F(3)) / F(3.0)        # q reads the binary16 round trip of E, the weight E itself


# ------------------------------------------------------------------------------------------------
# the host builder's list against the twin
# ------------------------------------------------------------------------------------------------
def quad(x0, z0, y, size, mat, uv_lo, uv_hi, base):
    """one quad facing down at height y: 2 triangles, UVs from uv_lo to uv_hi; base: the mesh's offset in the scene's material ids (Vertex.normal.w)"""
    v = np.array([[x0, y, z0, 0, -1, 0, base], [x0 + size, y, z0, 0, -1, 0, base], [x0 + size, y, z0 + size, 0, -1, 0, base], [x0, y, z0 + size, 0, -1, 0, base]], np.float32)
    idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    (a, b), (c, d) = uv_lo, uv_hi
    uv = np.array([(a, b), (c, b), (c, d), (a, b), (c, d), (a, d)], np.float32)
    return v, idx, np.full(6, mat, np.uint32), uv


def builder_world(black=False):
    """four materials (two mapped emitters: one sRGB 5 x 3, one linear 2 x 2; one unmapped emitter; one mapped non-emitter), three meshes, four instances — one mirrored and
    scaled, one hidden — and one triangle whose three material ids differ (it is no light, and a hit reads its first id)"""
    rng = np.random.default_rng(9)
    mats = np.zeros((4, 32), np.float32)
    mats[:, 0:3] = 0.5
    mats[0, 8:11] = (12.0, 10.0, 0.0); mats[1, 8:11] = (0.75, 0.75, 3.0); mats[2, 8:11] = (4.0, 4.0, 4.0)
    t0 = rng.integers(0, 256, (3, 5, 4), dtype=np.uint8); t1 = rng.integers(0, 256, (2, 2, 4), dtype=np.uint8)
    if black:
        t0[..., :3] = 0; t1[..., :3] = 0
    textures = [(t0, True), (t1, False)]
    a = quad(0.0, 0.0, 2.0, 1.0, 0, (-0.7, 0.1), (1.8, 0.9), 0)
    b = quad(2.0, 0.0, 2.0, 0.5, 1, (0.25, 0.25), (0.75, 0.75), 6)
    cv, ci, cm, cu = quad(4.0, 0.0, 2.0, 0.25, 2, (0, 0), (1, 1), 12)
    cm = cm.copy(); cm[3:6] = (0, 3, 3)                                        # the second triangle: mixed ids, first id an emitter with a map
    meshes = [a[:3], b[:3], (cv, ci, cm)]
    uvs = [a[3], b[3], cu]
    mirror = np.eye(4, dtype=np.float32); mirror[0, 0] = -2.0; mirror[3, 0] = -1.0; mirror[3, 2] = 3.0
    instances = [(0, EYE), (1, EYE), (2, EYE), (0, mirror.reshape(16)), (1, EYE)]
    return mats, meshes, uvs, instances, textures, ([0, 1, 0, 1] if black else [0, 1, -1, 1]), (4,)      # (black: every emitter mapped, so that no weight is left)


def write_world(path, mats, meshes, uvs, instances, textures, ke, hidden):
    out = [struct.pack("<I", len(mats)), np.asarray(mats, np.float32).tobytes(), struct.pack("<I", len(textures))]
    for px, srgb in textures:
        out += [struct.pack("<III", px.shape[1], px.shape[0], 1 if srgb else 0), np.ascontiguousarray(px).tobytes()]
    out.append(struct.pack("<I", len(meshes)))
    for (v, idx, mid), uv in zip(meshes, uvs):
        out += [struct.pack("<I", len(v)), np.asarray(v, np.float32).tobytes(), struct.pack("<I", len(idx)), np.asarray(idx, np.uint32).tobytes(), np.asarray(mid, np.uint32).tobytes()]
        out += [struct.pack("<I", 0)] if uv is None else [struct.pack("<I", 1), np.asarray(uv, np.float32).tobytes()]
    out.append(struct.pack("<I", len(instances)))
    for i, (mesh, m) in enumerate(instances):
        out += [struct.pack("<I", mesh), np.asarray(m, np.float32).tobytes(), struct.pack("<I", 1 if i in hidden else 0)]
    out.append(np.asarray(ke, np.int32).tobytes())
    path.write_bytes(b"".join(out))


@pytest.fixture(scope="module")
def builder_exe(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    pk = os.path.join(ROOT, "royaltracer-dx_amd")
    srcs = [os.path.join(ROOT, "tests", "sanitize", "emimap_main.cpp")] + [os.path.join(pk, "csrc", f) for f in ("rtx_scene_host.cpp", "rtx_small_scene.cpp", "rtx_bvh_build.cpp", "rtx_bvh_wide.cpp", "rtx_bvh_replay.cpp")]
    exe = str(tmp_path_factory.mktemp("emimap") / "san_emimap")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pk, "csrc"), "-pthread", "-o", exe] + srcs
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-3000:]
    return exe


def run_builder(exe, path):
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == "done", r.stdout[-1500:]
    words = lambda l: np.array([int(x, 16) for x in l.split()[1:]], np.uint32)
    return dict(active=int(lines[0].split()[1]), total=words(lines[1])[0], lights=np.array([words(l) for l in lines if l.startswith("L")], np.uint32).reshape(-1, 22),
                q=words([l for l in lines if l.startswith("Q")][0]))


@pytest.mark.parametrize("black", [False, True])
def test_host_builder_equals_the_twin(rt, builder_exe, tmp_path, black):
    mats, meshes, uvs, instances, textures, ke, hidden = builder_world(black)
    write_world(tmp_path / "w.bin", mats, meshes, uvs, instances, textures, ke, hidden)
    got = run_builder(builder_exe, tmp_path / "w.bin")
    L = em.LightList(rt.half_round, mats, meshes, uvs, instances, textures, ke, hidden)
    assert got["active"] == 1 and L.active
    assert len(L.records) == 7 == len(got["lights"])                           # 2 + 2 + 1 + 2 triangles: the mixed one and the hidden instance's are no lights
    assert np.array_equal(got["lights"][:, :20], bits(L.records)) and got["total"] == bits(L.total)
    assert np.array_equal(got["lights"][:, 20], L.prim) and np.array_equal(got["lights"][:, 21].view(np.int32), L.tex)
    assert np.array_equal(got["q"], bits(L.q)) and len(L.q) == 10
    assert (black or L.q[5] != 0) and (L.q[8:10] == 0).all()                              # the mixed triangle has a q (a hit reads its first id); the hidden instance has none
    if black:
        assert L.total == 0 and L.nlights == 0 and (L.records[:, 11] == 0).all() and L.records[-1, 3] == 1 and not L.q.any()
        return
    assert L.nlights == 7 and L.total > 0 and set(L.tex.tolist()) == {0, 1, -1}
    # the weights follow the texels, not area x mean(Ke): the order differs from the unmapped scene's
    U = em.LightList(rt.half_round, mats, meshes, uvs, instances, textures, [-1] * 4, hidden)
    assert not U.active and not U.q.any() and len(U.records) == 7 and not np.array_equal(U.records[:, 11], L.records[:, 11])
    write_world(tmp_path / "u.bin", mats, meshes, uvs, instances, textures, [-1] * 4, hidden)
    got = run_builder(builder_exe, tmp_path / "u.bin")
    assert got["active"] == 0 and np.array_equal(got["lights"][:, :20], bits(U.records)) and not got["lights"][:, 20:].any() and len(got["q"]) == 0
    # a map on a non-emitter alone activates nothing
    write_world(tmp_path / "n.bin", mats, meshes, uvs, instances, textures, [-1, -1, -1, 0], hidden)
    got = run_builder(builder_exe, tmp_path / "n.bin")
    assert got["active"] == 0 and np.array_equal(got["lights"][:, :20], bits(U.records)) and len(got["q"]) == 0


def test_all_255_linear_map_gives_the_unmapped_list(rt):
    mats, meshes, uvs, instances, textures, ke, hidden = builder_world()
    white = (np.full((3, 5, 4), 255, np.uint8), False)
    L = em.LightList(rt.half_round, mats, meshes, uvs, instances, [white, white], ke, hidden)
    U = em.LightList(rt.half_round, mats, meshes, uvs, instances, textures, [-1] * 4, hidden)
    assert L.active and np.array_equal(bits(L.records), bits(U.records)) and np.array_equal(bits(L.pdf_l), bits(U.pdf_l))
    kh = tr.half_round_array(rt.half_round, mats[:, 8:11])
    assert np.array_equal(bits(L.q[:2]), bits(np.repeat(((kh[0, 0] + kh[0, 1]) + kh[0, 2]) / F(3.0), 2)))


# ------------------------------------------------------------------------------------------------
# the host layer's loading
# ------------------------------------------------------------------------------------------------
def write_quad(tmp_path, mtl_lines):
    (tmp_path / "q.mtl").write_text("newmtl sign\nKd 0.8 0.8 0.8\n" + mtl_lines)
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 2 0 0\nv 2 2 0\nv 0 2 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nusemtl sign\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")
    return [str(tmp_path / "q.obj")], str(tmp_path) + "/"


def test_loader_binds_map_ke(rt, tmp_path):
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    (tmp_path / "glow.ppm").write_bytes(b"P6 3 5 255\n" + rgb.tobytes())
    rgb4 = np.dstack([rgb, np.full((5, 3, 1), 255, np.uint8)])
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ke glow.ppm\n"))
    n = len(sc.materials)
    assert len(sc.ke_maps) == n and sc.ke_maps[-1] == sc.textures.index("glow.ppm") and all(t == -1 for t in sc.ke_maps[:-1])
    assert np.array_equal(sc.texture_pixels[sc.ke_maps[-1]], rgb4)
    # the unit-Ke rule: the file gives no Ke, the parser records zeros, the binding step sets them to one
    assert np.asarray(sc.materials, np.float32)[-1][8:11].tolist() == [1, 1, 1]
    # ... emission_maps=False leaves the record as parsed, and so does NO_TEXTURES
    for kw in (dict(emission_maps=False), dict(textures=False)):
        sc0 = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ke glow.ppm\n"), **kw)
        assert np.asarray(sc0.materials, np.float32)[-1][8:11].tolist() == [0, 0, 0] and all(t == -1 for t in sc0.ke_maps), kw
        assert sc0.material_ext[-1]["maps"]["Ke"] == "glow.ppm"                # (the parser's record of the statement stays)
    # a Ke the file does give is kept
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "Ke 4 0 0.5\nmap_Ke glow.ppm\n"))
    assert np.asarray(sc.materials, np.float32)[-1][8:11].tolist() == [4, 0, 0.5] and sc.ke_maps[-1] >= 0
    # a map whose image is missing is not bound, and the rule does not apply; the other loaders are untouched by the flag
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ke missing.ppm\n"))
    assert sc.ke_maps[-1] == -1 and np.asarray(sc.materials, np.float32)[-1][8:11].tolist() == [0, 0, 0]
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ke glow.ppm\nmap_Kd glow.ppm\n"), emission_maps=False)
    assert sc.material_maps[-1] == sc.textures.index("glow.ppm") and sc.ke_maps[-1] == -1


def test_golden_scenes_have_no_emission_maps(rt, golden_dir):
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    assert len(sc.ke_maps) == len(sc.materials) and all(m == -1 for m in sc.ke_maps)
    assert rt.Scene.cornell().ke_maps == [-1] * len(rt.Scene.cornell().materials)


# ------------------------------------------------------------------------------------------------
# the interface
# ------------------------------------------------------------------------------------------------
def test_new_symbols_exist(rt):
    L = rt.lib
    names = ("rtx_debug_emission", "rtx_debug_light_sample", "rtxh_scene_emission_map")
    for name in names:
        assert getattr(L, name)
    assert rt.MAP_KE == 12 and (rt.MAP_KS, rt.MAP_PR, rt.MAP_PM) == (6, 8, 10)
    for f in ("emission", "light_sample"):
        assert callable(getattr(rt.Context, f))
    assert L.rtx_debug_emission(None, None, 0, None) == -1 and L.rtx_debug_light_sample(None, None, 0, None) == -1
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("enum { RTX_MAP_KE = 12 };", "EMISSION MAPS", "int  rtx_debug_emission(rtx_ctx*, const float* hits4, uint32_t n, float* out8);",
                 "int  rtx_debug_light_sample(rtx_ctx*, const uint32_t* seeds2, uint32_t n, float* out12);", "Ke'[k] = half_round(m.KeFull[k] * tl[k])"):
        assert text in header, text
    host = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "#define RTXH_OBJ_NO_EMISSION_MAPS 128u" in host and "rtxh_scene_emission_map(" in host
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in names:
        assert f" T {name}\n" in nm, name
    usage = subprocess.run([os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render"), "--help"], capture_output=True, text=True).stdout
    assert "--no-emission-maps" in usage

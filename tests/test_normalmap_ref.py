"""Tangent-space normal maps without a GPU: the properties of the numpy twin (tests/normalmap_ref.py) that tests/test_normalmap.py holds the device to, the host layer's
loading of norm / map_Bump images, the new symbols, and the host header (csrc/rtx_normalmap_host.hpp) under the sanitizers as a stand-alone program compared with the twin
bit for bit."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import normalmap_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EYE = np.eye(4, dtype=np.float32).reshape(16)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def rep(a, k):
    return np.repeat(np.asarray(a, np.float32).reshape(1, -1), k, axis=0)


# an axis-aligned quad in the plane z = 0 with identity UVs: T = +x, B = +y, n = +z
QUAD_P = np.array([[[0, 0, 0], [1, 0, 0], [1, 1, 0]], [[0, 0, 0], [1, 1, 0], [0, 1, 0]]], np.float32)
QUAD_UV = QUAD_P[..., :2].copy()


# ------------------------------------------------------------------------------------------------
# the twin
# ------------------------------------------------------------------------------------------------
def test_decode_table():
    T = nr.table()
    assert T.dtype == np.float32 and T[128] == 0.0 and T[255] == 1.0 and T[0] == -1.0 and T[1] == -1.0 and T[2] < 0 and T[2] > -1.0
    assert (np.diff(T[1:]) > 0).all()
    for g in range(256):                                                 # FlipGreen is an exact negation under Nt
        g2 = 255 if g == 0 else 256 - g
        assert T[g2] == -T[g], g


def test_flat_texels_return_n_itself():
    rng = np.random.default_rng(1)
    k = 400
    n = unit(rng.normal(size=(k, 3))); wo = unit(rng.normal(size=(k, 3)))
    tan = rng.normal(size=(k, 6)).astype(np.float32); M = rng.normal(size=(k, 16)).astype(np.float32)
    c = np.zeros((k, 3), np.float32); c[:, 2] = rng.uniform(0.01, 1, k).astype(np.float32)
    br = {}
    out = nr.perturb(n, c, tan, M, wo, br)
    assert np.array_equal(bits(out), bits(n)) and br["flat"].all()
    # ... through the sampler: r = g = 128 texels with any b, at any (s, t)
    px = rng.integers(0, 256, (5, 3, 4), dtype=np.uint8); px[..., 0] = 128; px[..., 1] = 128; px[..., 2] = rng.integers(129, 256, (5, 3))
    s, t = rng.uniform(-2, 2, k).astype(np.float32), rng.uniform(-2, 2, k).astype(np.float32)
    c = nr.decode(px, s, t)
    assert (c[:, 0] == 0).all() and (c[:, 1] == 0).all() and (c[:, 2] > 0).all()
    assert np.array_equal(bits(nr.perturb(n, c, tan, M, wo)), bits(n))


def test_unit_length_and_viewer_side():
    """| |n'|^2 - 1 | <= 1e-5 (a float32 normalisation is good to a few ulp, ~7e-7; the bound is ~14 times that) and dot(n', wo) has the sign of dot(n, wo)"""
    rng = np.random.default_rng(2)
    k = 20000
    n = unit(rng.normal(size=(k, 3))); wo = unit(rng.normal(size=(k, 3)))
    tan = rng.normal(size=(k, 6)).astype(np.float32)
    M = rep(EYE, k).copy(); M[:, :12] += rng.normal(scale=0.5, size=(k, 12)).astype(np.float32)
    T = nr.table()
    c = T[rng.integers(0, 256, (k, 3))]
    br = {}
    out = nr.perturb(n, c, tan, M, wo, br)
    l2 = (out.astype(np.float64) ** 2).sum(axis=1)
    assert np.abs(l2 - 1.0).max() <= 1e-5
    a = (n[:, 0] * wo[:, 0] + n[:, 1] * wo[:, 1]) + n[:, 2] * wo[:, 2]
    ap = (out[:, 0] * wo[:, 0] + out[:, 1] * wo[:, 1]) + out[:, 2] * wo[:, 2]
    assert np.array_equal(np.sign(a), np.sign(ap))
    assert br["guard"].sum() > 100 and (~br["guard"] & ~br["flat"]).sum() > 100          # both sides of the guard are exercised
    assert np.array_equal(bits(out[br["guard"]]), bits(n[br["guard"]]))


def _tilt(p3, uv3, c, M=EYE, n=(0, 0, 1), wo=(0, 0, 1)):
    tan = nr.tangent_records(p3, uv3)
    k = len(tan)
    return nr.perturb(rep(n, k), rep(c, k), tan, rep(M, k), rep(wo, k))


def test_tilt_directions_on_a_quad():
    tan = nr.tangent_records(QUAD_P, QUAD_UV)
    assert np.array_equal(tan, rep([1, 0, 0, 0, 1, 0], 2))
    T = nr.table()
    cx = _tilt(QUAD_P, QUAD_UV, [T[219], 0, T[219]])
    assert (cx[:, 0] > 0.5).all() and (cx[:, 1] == 0).all() and (cx[:, 2] > 0.5).all()      # c.x > 0 tilts towards +T
    cy = _tilt(QUAD_P, QUAD_UV, [0, T[219], T[219]])
    assert (cy[:, 1] > 0.5).all() and (cy[:, 0] == 0).all() and (cy[:, 2] > 0.5).all()      # c.y > 0 tilts towards +B
    cm = _tilt(QUAD_P, QUAD_UV, [T[37], 0, T[219]])
    assert (cm[:, 0] < -0.5).all()


def test_mirrored_instance_flips_the_mirrored_axis_only():
    T = nr.table()
    M = EYE.copy(); M[0] = -1.0                                          # o2w = diag(-1, 1, 1)
    c = [T[200], T[180], T[230]]
    a = _tilt(QUAD_P, QUAD_UV, c)
    b = _tilt(QUAD_P, QUAD_UV, c, M=M)
    assert (a[:, 0] > 0).all() and (b[:, 0] < 0).all() and np.array_equal(bits(a[:, 0]), bits(-b[:, 0]))
    assert (a[:, 1] > 0).all() and np.array_equal(bits(a[:, 1]), bits(b[:, 1])) and np.array_equal(bits(a[:, 2]), bits(b[:, 2]))


def test_mirrored_uvs_keep_the_world_space_tilt():
    """the same texel layout in world space, reached through UVs that run the other way along x (u = 1 - x) and a texel whose red channel is negated accordingly: the geometry,
    not the winding of the UVs, decides the handedness"""
    T = nr.table()
    uvm = QUAD_UV.copy(); uvm[..., 0] = 1.0 - uvm[..., 0]
    tan = nr.tangent_records(QUAD_P, uvm)
    assert np.array_equal(tan, rep([-1, 0, 0, 0, 1, 0], 2))
    a = _tilt(QUAD_P, QUAD_UV, [T[200], T[180], T[230]])
    b = _tilt(QUAD_P, uvm, [T[56], T[180], T[230]])                      # byte 56 = 256 - 200: the image mirrored along u stores -x
    assert np.array_equal(bits(a), bits(b))
    # and with the UVs alone mirrored the green tilt (along the unmirrored v) keeps its world direction
    g = _tilt(QUAD_P, uvm, [0, T[200], T[230]])
    assert (g[:, 1] > 0).all() and (g[:, 0] == 0).all()


def test_degenerate_uvs_give_zero_records_and_n():
    rng = np.random.default_rng(3)
    p = rng.normal(size=(4, 3, 3)).astype(np.float32)
    uv = np.zeros((4, 3, 2), np.float32)                                 # no UVs
    uv[1] = [[0.1, 0.1], [0.2, 0.2], [0.4, 0.4]]                         # collinear
    uv[2] = [[0.3, 0.7], [0.3, 0.7], [0.9, 0.1]]                         # two corners coincide
    uv[3] = [[0, 0], [1, 0], [0, 1]]                                     # a proper one
    tan = nr.tangent_records(p, uv)
    assert not tan[:3].any() and tan[3].any()
    n = unit(rng.normal(size=(4, 3))); wo = n.copy()
    br = {}
    out = nr.perturb(n, rep([0.5, 0.25, 0.8], 4), tan, rep(EYE, 4), wo, br)
    assert np.array_equal(bits(out[:3]), bits(n[:3])) and br["degenerate"][:3].all() and not br["degenerate"][3]
    assert not np.array_equal(bits(out[3]), bits(n[3]))
    # positions beyond float32 after the division, and a determinant that underflows: zeros, never inf or nan
    big = np.array([[[0, 0, 0], [1e30, 0, 0], [0, 1e30, 0]]], np.float32)
    assert not nr.tangent_records(big, np.array([[[0, 0], [1e-10, 0], [0, 1e-10]]], np.float32)).any()
    tiny = nr.tangent_records(QUAD_P[:1], np.array([[[0, 0], [1e-30, 0], [1e-30, 1e-30]]], np.float32))
    assert np.isfinite(tiny).all()


def test_height_map_conversion():
    flat = np.full((4, 6, 4), 77, np.uint8)
    out = nr.height_to_normal(flat, 5.0)
    assert (out[..., :2] == 128).all() and (out[..., 2:] == 255).all()
    # a ramp that rises with x: the normal leans towards -x (c.x < 0 -> byte < 128); rows rising towards the TOP (v upward): leans towards -y
    ramp = np.zeros((8, 8, 4), np.uint8); ramp[..., 0] = (np.arange(8) * 20)[None, :]
    out = nr.height_to_normal(ramp, 4.0)
    assert (out[:, 1:7, 0] < 128).all() and (out[:, 1:7, 1] == 128).all()
    ramp = np.zeros((8, 8, 4), np.uint8); ramp[..., 0] = (np.arange(8)[::-1] * 20)[:, None]
    out = nr.height_to_normal(ramp, 4.0)
    assert (out[1:7, :, 1] < 128).all() and (out[1:7, :, 0] == 128).all()
    one = nr.height_to_normal(np.full((1, 1, 4), 9, np.uint8), 100.0)      # 1 x 1: its own neighbour on every side
    assert one.tolist() == [[[128, 128, 255, 255]]]


# ------------------------------------------------------------------------------------------------
# the host layer's loading
# ------------------------------------------------------------------------------------------------
def write_quad(tmp_path, mtl_lines):
    (tmp_path / "q.mtl").write_text("newmtl wall\nKd 0.8 0.8 0.8\n" + mtl_lines)
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 2 0 0\nv 2 2 0\nv 0 2 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nusemtl wall\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")
    return [str(tmp_path / "q.obj")], str(tmp_path) + "/"


def test_loader_binds_norm_and_bump_on_request(rt, tmp_path):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    (tmp_path / "n.ppm").write_bytes(b"P6 3 5 255\n" + rgb.tobytes())
    (tmp_path / "h.pgm").write_bytes(b"P5 6 4 255\n" + grey.tobytes())
    wall = lambda sc: sc.normal_maps[-1]
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm n.ppm\n"))
    assert wall(sc) == sc.textures.index("n.ppm") and np.array_equal(sc.texture_pixels[wall(sc)][..., :3], rgb) and len(sc.normal_maps) == len(sc.materials)
    assert all(m == -1 for m in sc.normal_maps[:-1])
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm n.ppm\n"), flip_y=True)
    assert np.array_equal(sc.texture_pixels[wall(sc)], nr.flip_green(np.dstack([rgb, np.full((5, 3, 1), 255, np.uint8)])))
    for kw in (dict(normal_maps=False), dict(textures=False)):
        sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm n.ppm\n"), **kw)
        assert all(m == -1 for m in sc.normal_maps)
    # map_Bump / bump: nothing by default; as a normal map or as a height map on request; a norm wins
    files = write_quad(tmp_path, "map_Bump h.pgm\n")
    assert wall(rt.Scene.from_obj(*files)) == -1
    h4 = np.dstack([grey, grey, grey, np.full_like(grey, 255)])
    sc = rt.Scene.from_obj(*files, bump="normal")
    assert wall(sc) >= 0 and np.array_equal(sc.texture_pixels[wall(sc)], h4)
    sc = rt.Scene.from_obj(*files, bump=4.0)
    assert wall(sc) >= 0 and np.array_equal(sc.texture_pixels[wall(sc)], nr.height_to_normal(h4, 4.0))
    sc = rt.Scene.from_obj(*files, bump=4.0, flip_y=True)
    assert np.array_equal(sc.texture_pixels[wall(sc)], nr.flip_green(nr.height_to_normal(h4, 4.0)))
    assert wall(rt.Scene.from_obj(*files, bump=4.0, normal_maps=False)) == -1
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm n.ppm\nbump h.pgm\n"), bump=4.0)
    assert wall(sc) == sc.textures.index("n.ppm") and np.array_equal(sc.texture_pixels[wall(sc)][..., :3], rgb)
    # an image another slot reads too is left alone: the converted map is a copy appended behind the files' textures, whose ids keep their order
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Kd h.pgm\nmap_Bump h.pgm\n"), bump=2.0)
    kd = sc.material_maps[-1]
    assert kd == sc.textures.index("h.pgm") and wall(sc) == len(sc.textures) - 1 and wall(sc) != kd
    assert np.array_equal(sc.texture_pixels[kd], h4) and np.array_equal(sc.texture_pixels[wall(sc)], nr.height_to_normal(h4, 2.0))
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm missing.ppm\n"))
    assert wall(sc) == -1


def test_golden_scenes_have_no_normal_maps(rt, golden_dir):
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    assert len(sc.normal_maps) == len(sc.materials) and all(m == -1 for m in sc.normal_maps)
    assert rt.Scene.cornell().normal_maps == [-1] * len(rt.Scene.cornell().materials)


# ------------------------------------------------------------------------------------------------
# the interface, the host code under the sanitizers
# ------------------------------------------------------------------------------------------------
def test_new_symbols_exist(rt):
    L = rt.lib
    names = ("rtx_debug_shading_normal", "rtx_debug_tri_tangents", "rtxh_scene_from_obj_ex2", "rtxh_scene_normal_map")
    for name in names:
        assert getattr(L, name)
    assert rt.MAP_NORMAL == 4 and rt.MAP_OPACITY == 2 and rt.MAP_KD == 0 and callable(rt.Context.shading_normal) and callable(rt.Context.tri_tangents)
    assert L.rtx_debug_shading_normal(None, None, None, 0, None) == -1 and L.rtx_debug_tri_tangents(None, 0, 0, None) == -1
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("enum { RTX_MAP_NORMAL = 4 };", "enum { RTX_MAP_KD = 0, RTX_MAP_OPACITY = 2 };", "int  rtx_debug_shading_normal(", "int  rtx_debug_tri_tangents(", "NORMAL MAPS",
                 "Nt[b] = max(((float)b - 128.0f) / 127.0f, -1.0f)", "a flat texel changes NOTHING"):
        assert text in header, text
    host = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "rtxh_scene_from_obj_ex2(" in host and "rtxh_scene_normal_map(" in host
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in names:
        assert f" T {name}\n" in nm, name
    usage = subprocess.run([os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render"), "--help"], capture_output=True, text=True).stdout
    for flag in ("--no-normal-maps", "--bump-height", "--bump-as-normal", "--normal-flip-y"):
        assert flag in usage, flag


def test_normalmap_host_header_under_asan_ubsan(tmp_path):
    """csrc/rtx_normalmap_host.hpp as a stand-alone program (tests/sanitize/normalmap_main.cpp: its own main, this header only) compiled with -fsanitize=address,undefined and
    run as a child process with nothing preloaded; its tangent records, converted height maps and flipped images equal the twin's bit for bit (double + - * / sqrt floor are
    IEEE in both)"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "san_normalmap")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "royaltracer-dx_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sanitize", "normalmap_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    rng = np.random.default_rng(12)
    p = rng.normal(size=(40, 3, 3)).astype(np.float32); uv = rng.uniform(-2, 2, (40, 3, 2)).astype(np.float32)
    uv[0] = 0                                                            # det = 0: no UVs
    uv[1] = [[0.1, 0.1], [0.2, 0.2], [0.4, 0.4]]                         # det = 0: collinear
    uv[2, 1] = uv[2, 0]                                                  # det = 0: two corners coincide
    uv[3] = [[0, 0], [1e-30, 0], [1e-30, 1e-30]]                         # a determinant that underflows float32 (1e-60: a double still holds it)
    uv[4] = [[0, 0], [1e-40, 0], [0, 1e-40]]                             # float32 denormals
    p[5] = [[0, 0, 0], [1e30, 0, 0], [0, 1e30, 0]]; uv[5] = [[0, 0], [1e-10, 0], [0, 1e-10]]      # 1e40: not finite as float32 -> zeros
    p[6] = [[1e30, -1e30, 1e30], [-1e30, 1e30, 3e38], [3e38, -3e38, 0]]
    p[7] = QUAD_P[0]; uv[7] = QUAD_UV[0]
    imgs = [(rng.integers(0, 256, (1, 1, 4), dtype=np.uint8), 3.0), (rng.integers(0, 256, (3, 5, 4), dtype=np.uint8), 4.0),
            (rng.integers(0, 256, (7, 2, 4), dtype=np.uint8), 0.25), (rng.integers(0, 256, (6, 6, 4), dtype=np.uint8), 1000.0), (np.full((2, 3, 4), 0, np.uint8), 1.0)]
    imgs[1][0][0, :, 1] = [0, 1, 128, 255, 2]                            # every special green byte of the flip
    blob = struct.pack("<I", len(p)) + b"".join(p[i].tobytes() + uv[i].tobytes() for i in range(len(p))) + struct.pack("<I", len(imgs))
    for px, s in imgs:
        blob += struct.pack("<IId", px.shape[1], px.shape[0], s) + px.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    assert lines[len(p) + 2 * len(imgs)] == "done", r.stdout[-500:]
    got = np.array([[float.fromhex(w) for w in l.split()[1:]] for l in lines[:len(p)]], np.float64).astype(np.float32)
    want = nr.tangent_records(p, uv)
    assert np.array_equal(bits(got), bits(want))
    assert not want[[0, 1, 2, 5]].any() and want[7].tolist() == [1, 0, 0, 0, 1, 0] and want[3].any() and np.isfinite(want).all()
    for i, (px, s) in enumerate(imgs):
        hl, gl = lines[len(p) + 2 * i], lines[len(p) + 2 * i + 1]
        assert hl[:2] == "H " and gl[:2] == "G "
        assert bytes.fromhex(hl[2:]) == nr.height_to_normal(px, s).tobytes(), i
        assert bytes.fromhex(gl[2:]) == nr.flip_green(px).tobytes(), i

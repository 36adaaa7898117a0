"""Alpha cut-outs without a GPU: the properties of the numpy twin (tests/cutout_ref.py) that tests/test_cutout.py holds the device to, the host layer's loading of map_d images
(alpha byte = the file's own alpha channel for a 32-bit TGA, else its first channel; one texture for a file that serves both slots; --kd-alpha), the new symbols, and the host
code under the sanitizers as a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cutout_ref as cr
import texture_ref as tr
from test_texture_ref import tga_bytes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the twin
# ------------------------------------------------------------------------------------------------
def test_four_equal_taps_are_exact():
    """a constant alpha byte b gives (float)b / 255.0f exactly at any (s, t): top = a + fx * 0, a + fy * 0"""
    rng = np.random.default_rng(1)
    s, t = rng.uniform(-3, 3, 500).astype(np.float32), rng.uniform(-3, 3, 500).astype(np.float32)
    for b in (0, 1, 127, 128, 200, 255):
        px = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8); px[..., 3] = b
        a = cr.alpha(px, s, t)
        assert np.array_equal(bits(a), bits(np.full(500, F(b) / F(255.0), np.float32)))
        assert cr.alpha_taps_agree(px, s, t).all()


def test_comparison_is_greater_or_equal():
    """byte 128 (128 / 255 = 0.50196...) is opaque, byte 127 (0.49803...) is not; and the boundary value 0.5f itself is accepted"""
    z = np.zeros(1, np.float32)
    for b, want in ((128, True), (127, False), (255, True), (0, False)):
        px = np.zeros((2, 2, 4), np.uint8); px[..., 3] = b
        assert bool(cr.accepted(cr.alpha(px, z, z))[0]) == want, b
    assert cr.accepted(np.array([0.5], np.float32))[0] and not cr.accepted(np.array([np.nextafter(F(0.5), F(0))], np.float32))[0]
    # alpha 0 | 255 side by side, sampled on the texel edge: fx = 0.5 exactly, a = 0 + 0.5 * (1 - 0) = 0.5f -> accepted
    px = np.zeros((1, 2, 4), np.uint8); px[0, 1, 3] = 255
    a = cr.alpha(px, np.array([0.5], np.float32), z)
    assert a[0] == F(0.5) and cr.accepted(a)[0]


def test_wrap_at_zero_one_and_negative():
    rng = np.random.default_rng(2)
    px = rng.integers(0, 256, (6, 5, 4), dtype=np.uint8)
    s, t = (rng.integers(0, 1024, 300) / 1024.0).astype(np.float32), (rng.integers(0, 1024, 300) / 1024.0).astype(np.float32)      # multiples of 2^-10: a whole shift is exact
    base = cr.alpha(px, s, t)
    assert len(np.unique(bits(base))) > 50
    for ds, dt in ((1, 0), (0, 1), (-1, -2), (3, -3)):
        assert np.array_equal(bits(cr.alpha(px, s + F(ds), t + F(dt))), bits(base))
    # s = 0 and s = 1 are the same place: the seam between the last and the first column
    assert np.array_equal(bits(cr.alpha(px, np.array([0.0, -0.0], np.float32), np.array([0.25, 0.25], np.float32))), bits(cr.alpha(px, np.array([1.0, -1.0], np.float32), np.array([0.25, -0.75], np.float32))))
    seam = cr.alpha(px, np.zeros(1, np.float32), np.array([1.0 - 0.5 / 6], np.float32))[0]             # row 0's centre: fy = 0, fx = 0.5 between columns 4 and 0
    T = tr.table(False)
    assert seam == T[px[0, 4, 3]] + F(0.5) * (T[px[0, 0, 3]] - T[px[0, 4, 3]])


def test_v_runs_upward():
    px = np.zeros((4, 4, 4), np.uint8); px[0, :, 3] = 255                                  # the TOP row is opaque
    s = np.full(2, 0.375, np.float32)
    a = cr.alpha(px, s, np.array([1.0 - 0.125, 0.125], np.float32))                        # t near 1 = top, t near 0 = bottom
    assert a[0] == F(1.0) and a[1] == F(0.0)


def test_alpha_is_linear_even_for_an_srgb_texture():
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    s, t = rng.uniform(-1, 2, 200).astype(np.float32), rng.uniform(-1, 2, 200).astype(np.float32)
    a = cr.alpha(px, s, t)
    # the colour sampler on a texture whose RED byte is this alpha: equal with the linear table, different with the sRGB one
    red = px.copy(); red[..., 0] = px[..., 3]
    assert np.array_equal(bits(a), bits(tr.sample(red, False, s, t)[:, 0])) and not np.array_equal(bits(a), bits(tr.sample(red, True, s, t)[:, 0]))


def test_cut_out_triangles_and_the_probe_form():
    mats = np.zeros((4, 32), np.float32); mats[2, 9] = 1.0                                 # material 2 emits
    assert list(cr.emits(mats)) == [False, False, True, False]
    tc = cr.cut_textures(mats, [0, -1, 1, None], [0, 1, 2, 3, 0])
    assert list(tc) == [0, -1, -1, -1, 0]
    px = np.zeros((2, 2, 4), np.uint8); px[..., 3] = 51
    hits = np.zeros((3, 4), np.float32); hits[:, 3].view(np.uint32)[:] = [0, 1, 0xFFFFFFFF]
    out = cr.opacity_probe([px], tc, np.zeros((5, 3, 2), np.float32), hits)
    assert out[0, 0] == F(51) / F(255.0) and out[0, 1:].view(np.uint32)[0] == 0
    assert (out[1:, 0] == 1.0).all() and (out[1:, 1].view(np.uint32) == 0xFFFFFFFF).all()


# ------------------------------------------------------------------------------------------------
# the loader
# ------------------------------------------------------------------------------------------------
CARD_OBJ = """mtllib card.mtl
v -2 0 -1
v 2 0 -1
v 2 3 -1
v -2 3 -1
v -1 0.2 0.5
v 1 0.2 0.5
v 1 2.2 0.5
v -1 2.2 0.5
v -0.5 2.9 0.5
v 0.5 2.9 0.5
v 0.5 2.9 1.5
v -0.5 2.9 1.5
v -2 0 3
v 2 0 3
vt 0 0
vt 1 0
vt 1 1
vt 0 1
usemtl wall
f 1/1 2/2 3/3 4/4
f 13/1 14/2 2/3 1/4
usemtl leaf
f 5/1 6/2 7/3 8/4
usemtl lamp
f 9 12 11 10
"""


def card_mtl(leaf):
    return "newmtl wall\nKd 0.2 0.7 0.9\nnewmtl leaf\nKd 0.9 0.3 0.1\n" + leaf + "newmtl lamp\nKd 0 0 0\nKe 12 11 10\n"


def write_card(d, leaf):
    (d / "card.mtl").write_text(card_mtl(leaf))
    (d / "card.obj").write_text(CARD_OBJ)
    return [str(d / "card.obj")], str(d) + "/"


def leaf_mask(rng, h=16, w=16):
    """an opacity mask of 4 x 4-texel blocks, half of them clear"""
    blocks = rng.integers(0, 2, (h // 4, w // 4), dtype=np.uint8) * 255
    blocks[0, 0], blocks[0, 1] = 0, 255
    return np.ascontiguousarray(np.repeat(np.repeat(blocks, 4, 0), 4, 1))


def test_map_d_as_pgm(rt, tmp_path):
    """map_d names a PGM: the texture's alpha byte is the grey value (and so are r, g, b); materials without map_d have no opacity map"""
    mask = leaf_mask(np.random.default_rng(5))
    (tmp_path / "mask.pgm").write_bytes(b"P5 16 16 255\n" + mask.tobytes())
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d mask.pgm\n"))
    assert sc.textures == ["mask.pgm"] and sc.material_maps == [-1, -1, -1, -1] and sc.opacity_maps == [-1, -1, 0, -1]
    assert np.array_equal(sc.texture_pixels[0], np.repeat(mask[..., None], 4, axis=2))
    # a PPM: the first (red) channel; colour bytes stay
    rgb = np.random.default_rng(6).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    (tmp_path / "mask.ppm").write_bytes(b"P6 16 16 255\n" + rgb.tobytes())
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d mask.ppm\n"))
    assert sc.opacity_maps == [-1, -1, 0, -1] and np.array_equal(sc.texture_pixels[0][..., :3], rgb) and np.array_equal(sc.texture_pixels[0][..., 3], rgb[..., 0])
    # a 24-bit TGA likewise
    img = np.random.default_rng(7).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    (tmp_path / "mask.tga").write_bytes(tga_bytes(img, 24, False, True))
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d mask.tga\n"))
    assert np.array_equal(sc.texture_pixels[0][..., :3], img[..., :3]) and np.array_equal(sc.texture_pixels[0][..., 3], img[..., 0])
    # cutouts=False: the scene of before (the name stays in the table, nothing is decoded or bound); a missing file is skipped
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d mask.pgm\n"), cutouts=False)
    assert sc.textures == ["mask.pgm"] and sc.texture_pixels == [None] and sc.opacity_maps == [-1, -1, -1, -1]
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d nothing.pgm\n"))
    assert sc.texture_pixels == [None] and sc.opacity_maps == [-1, -1, -1, -1]
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_d mask.pgm\n"), textures=False)
    assert sc.texture_pixels == [None] and sc.opacity_maps == [-1, -1, -1, -1]


def test_one_32_bit_tga_for_both_slots(rt, tmp_path):
    """map_Kd and map_d name the same 32-bit TGA: ONE texture, bound to both slots, its alpha the file's own"""
    img = np.random.default_rng(8).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    (tmp_path / "leaf.tga").write_bytes(tga_bytes(img, 32, True, False))
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_Kd leaf.tga\nmap_d leaf.tga\n"))
    assert sc.textures == ["leaf.tga"] and sc.material_maps == [-1, -1, 0, -1] and sc.opacity_maps == [-1, -1, 0, -1]
    assert np.array_equal(sc.texture_pixels[0], img)
    # two files: two textures; the map_Kd image keeps the alpha it always had (255 for a file without one)
    (tmp_path / "col.ppm").write_bytes(b"P6 16 16 255\n" + img[..., :3].tobytes())
    (tmp_path / "mask.pgm").write_bytes(b"P5 16 16 255\n" + img[..., 3].tobytes())
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_Kd col.ppm\nmap_d mask.pgm\n"))
    assert sc.textures == ["col.ppm", "mask.pgm"] and sc.material_maps == [-1, -1, 0, -1] and sc.opacity_maps == [-1, -1, 1, -1]
    assert (sc.texture_pixels[0][..., 3] == 255).all() and np.array_equal(sc.texture_pixels[1][..., 3], img[..., 3])


def test_kd_alpha_is_opt_in(rt, tmp_path):
    """a 32-bit map_Kd without a map_d: nothing by default, the texture's own alpha with kd_alpha; a 24-bit map_Kd never; a map_d wins"""
    img = np.random.default_rng(9).integers(0, 256, (16, 16, 4), dtype=np.uint8)
    (tmp_path / "leaf.tga").write_bytes(tga_bytes(img, 32, False, True))
    (tmp_path / "flat.tga").write_bytes(tga_bytes(img, 24, False, True))
    (tmp_path / "mask.pgm").write_bytes(b"P5 16 16 255\n" + img[..., 1].tobytes())
    files = write_card(tmp_path, "map_Kd leaf.tga\n")
    sc = rt.Scene.from_obj(*files)
    assert sc.material_maps == [-1, -1, 0, -1] and sc.opacity_maps == [-1, -1, -1, -1] and np.array_equal(sc.texture_pixels[0], img)
    sc = rt.Scene.from_obj(*files, kd_alpha=True)
    assert sc.material_maps == [-1, -1, 0, -1] and sc.opacity_maps == [-1, -1, 0, -1] and np.array_equal(sc.texture_pixels[0], img)
    sc = rt.Scene.from_obj(*files, kd_alpha=True, cutouts=False)
    assert sc.opacity_maps == [-1, -1, -1, -1]
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_Kd flat.tga\n"), kd_alpha=True)
    assert sc.opacity_maps == [-1, -1, -1, -1] and (sc.texture_pixels[0][..., 3] == 255).all()
    sc = rt.Scene.from_obj(*write_card(tmp_path, "map_Kd leaf.tga\nmap_d mask.pgm\n"), kd_alpha=True)
    assert sc.opacity_maps == [-1, -1, 1, -1] and np.array_equal(sc.texture_pixels[0], img)


def test_golden_scenes_have_no_opacity_maps(rt, golden_dir):
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    assert len(sc.opacity_maps) == len(sc.materials) and all(m == -1 for m in sc.opacity_maps)
    for sub in ("mtlext", "objfuzz"):
        d = os.path.join(golden_dir, sub)
        for f in sorted(os.listdir(d)):
            if f.endswith(".obj"):
                sc = rt.Scene.from_obj([os.path.join(d, f)], d + "/")
                assert all(m == -1 for m in sc.opacity_maps), f
                sc = rt.Scene.from_obj([os.path.join(d, f)], d + "/", kd_alpha=True)
                assert all(m == -1 for m in sc.opacity_maps), f
    assert rt.Scene.cornell().opacity_maps == [-1] * len(rt.Scene.cornell().materials)


# ------------------------------------------------------------------------------------------------
# the interface, the host code under the sanitizers
# ------------------------------------------------------------------------------------------------
def test_new_symbols_exist(rt):
    L = rt.lib
    for name in ("rtx_debug_opacity", "rtxh_scene_from_obj_ex", "rtxh_scene_opacity_map"):
        assert getattr(L, name)
    assert rt.MAP_OPACITY == 2 and rt.MAP_KD == 0 and callable(rt.Context.opacity)
    assert L.rtx_debug_opacity(None, None, 0, None) == -1
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("enum { RTX_MAP_KD = 0, RTX_MAP_OPACITY = 2 };", "int  rtx_debug_opacity(", "ALPHA CUT-OUTS", "ACCEPTED iff a >= 0.5f", "rtx_render_v6_pass1, rtx_render_restir"):
        assert text in header, text
    host = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "rtxh_scene_from_obj_ex(" in host and "rtxh_scene_opacity_map(" in host
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in ("rtx_debug_opacity", "rtxh_scene_from_obj_ex", "rtxh_scene_opacity_map"):
        assert f" T {name}\n" in nm, name
    exe = os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render")
    usage = subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
    assert "--no-cutouts" in usage and "--kd-alpha" in usage


def test_cutout_host_code_under_asan_ubsan(tmp_path):
    """the reader's channel count, the alpha conversion and the host scene's opacity-map table as a stand-alone program (tests/sanitize/cutout_main.cpp, its own main) compiled
    with -fsanitize=address,undefined and run as a child process on good, truncated and corrupt files; nothing sanitized is loaded into this interpreter"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    from test_host_layer import _host_layer_sources
    pk = os.path.join(ROOT, "royaltracer-dx_amd")
    srcs = [os.path.join(ROOT, "tests", "sanitize", f) for f in ("cutout_main.cpp", "device_stubs.cpp")] + _host_layer_sources(pk)
    exe = str(tmp_path / "san_cutout")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(pk, "csrc"), "-I" + os.path.join(pk, "host"), "-pthread", "-o", exe] + srcs
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-2000:]
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (7, 11, 4), dtype=np.uint8)
    img[2:5, 3:9] = img[2, 3]
    good = {"g.pgm": b"P5 11 7 255\n" + img[..., 0].tobytes(), "c.ppm": b"P6\n# c\n11 7\n255\n" + img[..., :3].tobytes(),
            "t24.tga": tga_bytes(img, 24, False, True), "t32.tga": tga_bytes(img, 32, True, False), "r32.tga": tga_bytes(img, 32, False, True)}
    bad = {"trunc.pgm": b"P5 11 7 255\n" + bytes(20), "hdr.pgm": b"P5 11", "deep.ppm": b"P6 1 1 65535\n" + bytes(6), "trunc.tga": tga_bytes(img, 32, True, True)[:40],
           "short.tga": tga_bytes(img, 32, True, False)[:17], "over.tga": tga_bytes(img, 32, True, True)[:18] + bytes([0xFF] * 64), "junk.bin": bytes(range(200)), "empty.bin": b""}
    for name, data in {**good, **bad}.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([exe] + [str(tmp_path / n) for n in list(good) + list(bad)] + [str(tmp_path / "missing.tga")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    red, alpha = int(img[..., 0].astype(np.int64).sum()), int(img[..., 3].astype(np.int64).sum())
    assert lines[:5] == [f"ok 11 7 1 {red}", f"ok 11 7 3 {red}", f"ok 11 7 3 {red}", f"ok 11 7 4 {alpha}", f"ok 11 7 4 {alpha}"], r.stdout
    assert sum(l.startswith("refused: ") for l in lines) == len(bad) + 1 and "done" in lines, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]

"""Diffuse texture maps without a GPU: the properties of the numpy emulation the device is held to (tests/texture_ref.py), and the host layer that feeds it — the OBJ
loader keeping `vt` per corner without disturbing vertices, indices or material ids, the PPM / PGM / TGA readers, a scene whose texture file is missing, and the new
symbols of the C-ABI, the host layer and the Python binding."""
import os
import struct

import numpy as np
import pytest

import texture_ref as tr

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------
# the emulation
# ------------------------------------------------------------------------------------------------
def test_tables_end_points_and_monotony():
    for srgb in (False, True):
        T = tr.table(srgb)
        assert T.dtype == np.float32 and T[0] == 0.0 and T[255] == 1.0 and np.all(np.diff(T) > 0)
    lin, s = tr.table(False), tr.table(True)
    assert lin[51] == F(51) / F(255) and np.all(s[1:255] < lin[1:255])
    assert s[10] == F(10 / 255.0 / 12.92) and abs(float(s[128]) - 0.21586) < 1e-5       # the linear toe and a mid grey


def test_sample_with_four_equal_taps_is_exact():
    rng = np.random.default_rng(1)
    px = np.zeros((16, 24, 4), np.uint8)
    px[:, :] = (37, 201, 5, 9)
    uv = rng.uniform(-2, 3, (500, 2)).astype(np.float32)
    for srgb in (False, True):
        T = tr.table(srgb)
        got = tr.sample(px, srgb, uv[:, 0], uv[:, 1])
        assert np.array_equal(bits(got), bits(np.tile(T[[37, 201, 5]], (500, 1))))
    assert tr.taps_agree(px, uv[:, 0], uv[:, 1]).all()
    px[3, 4] = (0, 0, 0, 0)
    assert not tr.taps_agree(px, [F(4.6 / 24)], [F(1 - 3.4 / 16)]).all()


def test_wrap_at_zero_one_and_negative():
    rng = np.random.default_rng(2)
    px = rng.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    uv = rng.uniform(0, 1, (300, 2)).astype(np.float32)
    uv = np.round(uv * 64) / 64                                 # so that adding a whole number is exact
    base = tr.sample(px, True, uv[:, 0], uv[:, 1])
    for du, dv in ((1, 0), (0, 1), (-1, -2), (2, -1)):
        assert np.array_equal(bits(tr.sample(px, True, uv[:, 0] + F(du), uv[:, 1] + F(dv))), bits(base))
    # s = 0 and s = 1 both sit on the seam between the last and the first column: the two halves of the blend
    T = tr.table(False)
    mid = tr.sample(px, False, [F(0), F(1)], [F(0.5 / 5), F(0.5 / 5)])          # t half a texel above the bottom: the last row
    want = T[px[4, 6, :3]] + F(0.5) * (T[px[4, 0, :3]] - T[px[4, 6, :3]])
    assert np.array_equal(bits(mid[0]), bits(want)) and np.array_equal(bits(mid[1]), bits(want))
    # a tap index below zero wraps to the far side
    ix0, ix1, iy0, iy1, fx, fy = tr.taps(px.shape, [F(0.01)], [F(0.99)])
    assert (ix0[0], ix1[0], iy0[0], iy1[0]) == (6, 0, 4, 0)


def test_v_runs_upward():
    px = np.zeros((4, 4, 4), np.uint8)
    px[0, :, 0] = 255                                           # the TOP row is red
    T = tr.table(False)
    top = tr.sample(px, False, [F(0.5)], [F(1 - 0.5 / 4)])      # v near 1 = the top of the image
    bottom = tr.sample(px, False, [F(0.5)], [F(0.5 / 4)])
    assert top[0, 0] == T[255] and bottom[0, 0] == 0.0


def test_kd_prime_uses_the_package_rounding(rt):
    kd = np.array([0.73, 0.1234567, 1.0], np.float32)
    tl = np.array([[0.5, 0.3333, 1.0], [0.0, 1e-6, 0.999]], np.float32)
    got = tr.kd_prime(rt.half_round, kd, tl)
    for i in range(2):
        for k in range(3):
            assert got[i, k] == F(rt.half_round(float(F(rt.half_round(float(kd[k]))) * tl[i, k])))
    x = np.random.default_rng(3).uniform(0, 2, 4000).astype(np.float32)
    assert np.array_equal(bits(tr.half_round_array(rt.half_round, x)), bits(x.astype(np.float16).astype(np.float32)))      # binary16, round to nearest even


# ------------------------------------------------------------------------------------------------
# vt through the host layer
# ------------------------------------------------------------------------------------------------
OBJ = """mtllib m.mtl
v 0 0 0
v 1 0 0
v 1 1 0
v 0 1 0
v 0.5 1.5 0
v 2 0 0
v 2 1 0
vn 0 0 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vt 0.5 1.5
usemtl a
f 1/1 2/2 3/3
f 1/1/1 3/3/1 4/4/1
usemtl b
f -7/-5 -6/-4 -5/-3
f 1 2 3
f 1//1 2/2/1 3//1
f 1/1 2/2 3/3 4/4
f 1/1 2/2 3/3 5/5 4/4
f 2/2 6 7/3
"""
MTL = "newmtl a\nKd 0.8 0.2 0.2\nnewmtl b\nKd 0.2 0.8 0.2\nmap_Kd missing.ppm\n"


def write_obj(d, text, name="t.obj"):
    (d / "m.mtl").write_text(MTL)
    (d / name).write_text(text)
    return str(d / name)


def test_vt_is_kept_per_corner_and_changes_nothing_else(rt, tmp_path, capfd):
    sc = rt.Scene.from_obj([write_obj(tmp_path, OBJ)], str(tmp_path) + "/")
    assert "map_Kd skipped" in capfd.readouterr().err           # the missing file: one line, and the scene loads
    novt = "\n".join(l for l in OBJ.splitlines() if not l.startswith("vt ")) + "\n"
    import re
    novt = re.sub(r"(-?\d+)/-?\d+/(-?\d+)", r"\1//\2", novt)  # v/vt/vn -> v//vn
    novt = re.sub(r"(-?\d+)/-?\d+(?=[ \n])", r"\1", novt)     # v/vt -> v
    plain = rt.Scene.from_obj([write_obj(tmp_path, novt, "n.obj")], str(tmp_path) + "/")
    (v, i, m), (pv, pi, pm) = sc.meshes[0], plain.meshes[0]
    assert np.array_equal(bits(v), bits(pv)) and np.array_equal(i, pi) and np.array_equal(m, pm)
    assert plain.uvs[0] is not None and not plain.uvs[0].any()  # no vt anywhere: (0, 0) at every corner
    uv = sc.uvs[0]
    assert uv.shape == (len(i), 2)
    VT = np.array([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 1.5]], np.float32)
    pos_to_vt = {(0, 0): 0, (1, 0): 1, (1, 1): 2, (0, 1): 3, (0.5, 1.5): 4}
    tri = lambda t: (v[i[3 * t:3 * t + 3], :2], uv[3 * t:3 * t + 3])
    assert np.array_equal(tri(0)[1], VT[[0, 1, 2]])             # v/vt
    assert np.array_equal(tri(1)[1], VT[[0, 2, 3]])             # v/vt/vn
    assert np.array_equal(tri(2)[1], VT[[0, 1, 2]])             # negative indices: -5, -4, -3 of five vt lines
    assert not tri(3)[1].any()                                  # no vt at all
    assert np.array_equal(tri(4)[1], np.array([[0, 0], [1, 0], [0, 0]], np.float32))      # a corner without vt gets (0, 0)
    for t in (5, 6, 7, 8, 9):                                   # the quad (2 triangles) and the 5-gon (3): every corner carries the vt of its own vertex
        p, q = tri(t)
        for c in range(3):
            assert np.array_equal(q[c], VT[pos_to_vt[(float(p[c, 0]), float(p[c, 1]))]]), t
    assert np.array_equal(tri(10)[1], np.array([[1, 0], [0, 0], [1, 1]], np.float32))
    assert len(i) == 33
    assert sc.textures == ["missing.ppm"] and sc.texture_pixels == [None] and sc.material_maps == [-1, -1, 0]
    assert [e["maps"] for e in plain.material_ext] == [e["maps"] for e in sc.material_ext]


def test_golden_scenes_load_unchanged(rt, golden_dir):
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    assert all(t is None for t in sc.texture_pixels) and all(m == -1 or sc.texture_pixels[m] is None for m in sc.material_maps)
    assert [u.shape for u in sc.uvs] == [(len(i), 2) for _, i, _ in sc.meshes]


# ------------------------------------------------------------------------------------------------
# the image readers
# ------------------------------------------------------------------------------------------------
def tga_bytes(img, bpp, top_down, rle):
    h, w = img.shape[:2]
    rows = img if top_down else img[::-1]
    px = rows[..., [2, 1, 0, 3]][..., :bpp // 8].reshape(-1, bpp // 8)
    hdr = struct.pack("<BBBHHBHHHHBB", 0, 0, 10 if rle else 2, 0, 0, 0, 0, 0, w, h, bpp, (0x20 if top_down else 0) | (8 if bpp == 32 else 0))
    if not rle:
        return hdr + px.tobytes()
    out, k = bytearray(), 0
    while k < len(px):                                          # runs of equal pixels as repeat packets, the rest as raw packets of up to 3 (packets cross rows)
        run = 1
        while k + run < len(px) and run < 128 and np.array_equal(px[k + run], px[k]):
            run += 1
        if run > 1:
            out += bytes([0x80 | (run - 1)]) + px[k].tobytes(); k += run
        else:
            n = min(3, len(px) - k)
            out += bytes([n - 1]) + px[k:k + n].tobytes(); k += n
    return hdr + bytes(out)


def test_readers_against_arrays(rt, tmp_path):
    rng = np.random.default_rng(4)
    img = rng.integers(0, 256, (7, 11, 4), dtype=np.uint8)
    img[2:5, 3:9] = img[2, 3]                                   # runs for the RLE packets
    opaque = img.copy(); opaque[..., 3] = 255
    (tmp_path / "a.ppm").write_bytes(b"P6\n# a comment\n11 7\n255\n" + img[..., :3].tobytes())
    assert np.array_equal(rt.read_image(tmp_path / "a.ppm"), opaque)
    (tmp_path / "g.pgm").write_bytes(b"P5 11 7 255\n" + img[..., 0].tobytes())
    grey = np.repeat(img[..., :1], 4, axis=2); grey[..., 3] = 255
    assert np.array_equal(rt.read_image(tmp_path / "g.pgm"), grey)
    for bpp in (24, 32):
        for top_down in (False, True):
            for rle in (False, True):
                p = tmp_path / f"t{bpp}{int(top_down)}{int(rle)}.tga"
                p.write_bytes(tga_bytes(img, bpp, top_down, rle))
                assert np.array_equal(rt.read_image(p), img if bpp == 32 else opaque), (bpp, top_down, rle)
    for name, data in (("trunc.ppm", b"P6 11 7 255\n" + bytes(10)), ("deep.ppm", b"P6 1 1 65535\n" + bytes(6)), ("ascii.ppm", b"P3 1 1 255 1 2 3\n"),
                       ("trunc.tga", tga_bytes(img, 24, True, True)[:40]), ("png.png", b"\x89PNG\r\n\x1a\n" + bytes(32))):
        (tmp_path / name).write_bytes(data)
        with pytest.raises(rt.RtxError):
            rt.read_image(tmp_path / name)
    with pytest.raises(rt.RtxError):
        rt.read_image(tmp_path / "nothing.tga")


def test_scene_loads_its_map_kd(rt, tmp_path):
    """an MTL that names a P6 and a TGA: both decoded, the scene exposes them with the UVs and the map ids"""
    rng = np.random.default_rng(6)
    a, b = rng.integers(0, 256, (4, 6, 4), dtype=np.uint8), rng.integers(0, 256, (3, 5, 4), dtype=np.uint8)
    a[..., 3] = 255; b[..., 3] = 255
    (tmp_path / "a.ppm").write_bytes(b"P6 6 4 255\n" + a[..., :3].tobytes())
    (tmp_path / "b.tga").write_bytes(tga_bytes(b, 24, False, True))
    (tmp_path / "m.mtl").write_text("newmtl a\nKd 1 1 1\nmap_Kd a.ppm\nnewmtl b\nKd 1 1 1\nmap_Kd -s 1 1 1 b.tga\nmap_Ks gloss.png\n")
    (tmp_path / "t.obj").write_text(OBJ)
    sc = rt.Scene.from_obj([str(tmp_path / "t.obj")], str(tmp_path) + "/")
    assert sc.textures == ["a.ppm", "b.tga", "gloss.png"] and sc.material_maps == [-1, 0, 1]
    assert np.array_equal(sc.texture_pixels[0], a) and np.array_equal(sc.texture_pixels[1], b) and sc.texture_pixels[2] is None      # map_Ks is a name only


def test_new_symbols_exist(rt):
    L = rt.lib
    for name in ("rtx_set_mesh_uvs", "rtx_set_texture", "rtx_set_material_map", "rtx_debug_texture_sample", "rtx_debug_albedo",
                 "rtxh_scene_mesh_uvs", "rtxh_scene_texture_pixels", "rtxh_read_image"):
        assert getattr(L, name)
    for name in ("set_mesh_uvs", "set_texture", "set_material_map", "texture_sample", "albedo", "bind_maps"):
        assert callable(getattr(rt.Context, name))
    assert rt.TEX_SRGB == 1 and rt.MAP_KD == 0 and callable(rt.read_image)
    assert L.rtx_set_mesh_uvs(None, 0, None, 0) == -1 and L.rtx_set_texture(None, 0, None, 1, 1, 0) == -1 and L.rtx_set_material_map(None, 0, 0, -1) == -1
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtx.h")).read()
    assert "#define RTX_TEX_SRGB 1u" in header and "RTX_MAP_KD = 0" in header and "NO MIP LEVELS" in header

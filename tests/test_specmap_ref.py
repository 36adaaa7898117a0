"""Specular, roughness and metalness maps without a GPU: the properties of the numpy twin (tests/specmap_ref.py) that tests/test_specmap.py holds the device to, the host
layer's loading of map_Ks / map_Pr / map_Pm images with its zero-scalar rule, the new symbols, and the host header (csrc/rtx_specmap_host.hpp) under the sanitizers as a
stand-alone program compared with the twin bit for bit."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import specmap_ref as sr
import texture_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rgba(rng, h, w):
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------
# the twin
# ------------------------------------------------------------------------------------------------
def test_constant_map_equals_a_scaled_material(rt):
    """every tap reads one byte: the bilinear value is T[byte] exactly, so the primed value is half_round(table value * T[byte]) at any (s, t)"""
    rng = np.random.default_rng(1)
    k = 300
    s, t = rng.uniform(-3, 3, k).astype(np.float32), rng.uniform(-3, 3, k).astype(np.float32)
    T, Ts = tr.table(False), tr.table(True)
    for shape in ((1, 1), (5, 3), (64, 16)):
        px = np.zeros(shape + (4,), np.uint8); px[...] = [200, 90, 31, 7]
        ks = np.array([0.5, 0.25, 1.0], np.float32)
        for srgb, tab in ((False, T), (True, Ts)):
            got = sr.ks_prime(rt.half_round, ks, px, srgb, s, t)
            want = tr.half_round_array(rt.half_round, ks * np.array([tab[200], tab[90], tab[31]], np.float32))
            assert np.array_equal(bits(got), bits(np.repeat(want[None], k, 0)))
        pr = sr.pr_prime(rt.half_round, F(0.75), px, s, t)
        assert np.array_equal(bits(pr), bits(np.full(k, rt.half_round(float(F(0.75) * T[90])), np.float32)))
        pm = sr.pm_prime(rt.half_round, F(0.5), px, s, t)
        assert np.array_equal(bits(pm), bits(np.full(k, rt.half_round(float(F(0.5) * T[31])), np.float32)))


def test_all_255_map_is_the_identity(rt):
    rng = np.random.default_rng(2)
    k = 200
    s, t = rng.uniform(-3, 3, k).astype(np.float32), rng.uniform(-3, 3, k).astype(np.float32)
    px = np.full((5, 3, 4), 255, np.uint8)
    vals = tr.half_round_array(rt.half_round, rng.uniform(0, 1, (k, 5)).astype(np.float32))       # table values: binary16-rounded already
    for srgb in (False, True):                                                                   # (sRGB 255 decodes to exactly 1 too)
        assert np.array_equal(bits(sr.ks_prime(rt.half_round, vals[:, :3], px, srgb, s, t)), bits(vals[:, :3]))
    assert np.array_equal(bits(sr.pr_prime(rt.half_round, vals[:, 3], px, s, t)), bits(vals[:, 3]))
    assert np.array_equal(bits(sr.pm_prime(rt.half_round, vals[:, 4], px, s, t)), bits(vals[:, 4]))


def test_channels_are_green_and_blue_and_always_linear(rt):
    rng = np.random.default_rng(3)
    px = rgba(rng, 5, 3)
    k = 100
    s, t = rng.uniform(-2, 2, k).astype(np.float32), rng.uniform(-2, 2, k).astype(np.float32)
    lin = tr.sample(px, False, s, t)
    assert np.array_equal(bits(sr.channel(px, 1, s, t)), bits(lin[:, 1])) and np.array_equal(bits(sr.channel(px, 2, s, t)), bits(lin[:, 2]))
    grey = px.copy(); grey[..., 1] = grey[..., 0]; grey[..., 2] = grey[..., 0]                   # a grey image serves either slot
    assert np.array_equal(bits(sr.channel(grey, 1, s, t)), bits(sr.channel(grey, 2, s, t)))


def test_ess_table_rows():
    rng = np.random.default_rng(4)
    for rows in (2, 17, 256):
        A = rng.uniform(0.05, 1, (rows, 16)).astype(np.float32)
        nv = np.concatenate([rng.uniform(-0.5, 1.5, 200), [-1.0, 0.0, 1.0, 2.0]]).astype(np.float32)
        # wr == 0: the look-up is the row's own (a material whose LUT is that row)
        for r in (0, 1, rows // 2, rows - 1):
            pr = np.full(len(nv), F(r) / F(rows - 1), np.float32)
            r0, r1, wr = sr.ess_rows(pr, rows)
            if (pr * F(rows - 1) == F(r)).all():
                assert (r0 == r).all() and (wr == 0).all()
                assert np.array_equal(bits(sr.ess_table(A, pr, nv)), bits(sr.ess_lut(A[r], nv)))
        # Pr' > 1 and Pr' == 0 clamp to the end rows
        for pr, row in ((1.5, rows - 1), (7.0, rows - 1), (1.0, rows - 1), (0.0, 0)):
            got = sr.ess_table(A, np.full(len(nv), pr, np.float32), nv)
            assert np.array_equal(bits(got), bits(sr.ess_lut(A[row], nv))), (rows, pr)
        # rows first: any roughness equals the material whose LUT is the blended row
        for pr in rng.uniform(0, 1.2, 20).astype(np.float32):
            got = sr.ess_table(A, np.full(len(nv), pr, np.float32), nv)
            assert np.array_equal(bits(got), bits(sr.ess_lut(sr.blend_row(A, pr), nv)))
    assert sr.table_error(None, 0) is None and sr.table_error(None, 3) and sr.table_error(np.ones((1, 16)), 1) and sr.table_error(np.ones((257, 16)), 257)
    bad = np.ones((3, 16), np.float32); bad[2, 15] = np.inf
    assert sr.table_error(bad, 3) and sr.table_error(np.ones((3, 16)), 3) is None


def test_zero_scalar_rule_twin():
    r, ch = sr.zero_scalar_rule([0, 0, 0, 0, 0])
    assert r.tolist() == [1, 1, 1, 1, 1] and ch == (True, True, True)
    r, ch = sr.zero_scalar_rule([0, 0.5, 0, 0.25, 0])
    assert r.tolist() == [0, 0.5, 0, 0.25, 1] and ch == (False, False, True)


# ------------------------------------------------------------------------------------------------
# the host layer's loading
# ------------------------------------------------------------------------------------------------
def write_quad(tmp_path, mtl_lines):
    (tmp_path / "q.mtl").write_text("newmtl wall\nKd 0.8 0.8 0.8\n" + mtl_lines)
    (tmp_path / "q.obj").write_text("mtllib q.mtl\nv 0 0 0\nv 2 0 0\nv 2 2 0\nv 0 2 0\nvt 0 0\nvt 1 0\nvt 1 1\nvt 0 1\nvn 0 0 1\nusemtl wall\nf 1/1/1 2/2/1 3/3/1\nf 1/1/1 3/3/1 4/4/1\n")
    return [str(tmp_path / "q.obj")], str(tmp_path) + "/"


def test_loader_binds_the_three_maps(rt, tmp_path):
    rng = np.random.default_rng(5)
    rgb = rng.integers(0, 256, (5, 3, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (4, 6), dtype=np.uint8)
    (tmp_path / "orm.ppm").write_bytes(b"P6 3 5 255\n" + rgb.tobytes())
    (tmp_path / "g.pgm").write_bytes(b"P5 6 4 255\n" + grey.tobytes())
    rgb4 = np.dstack([rgb, np.full((5, 3, 1), 255, np.uint8)])
    g4 = np.dstack([grey, grey, grey, np.full_like(grey, 255)])
    # the three lists are filled; one file serves PR and PM
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ks g.pgm\nmap_Pr orm.ppm\nmap_Pm orm.ppm\n"))
    n = len(sc.materials)
    assert len(sc.ks_maps) == n and len(sc.pr_maps) == n and len(sc.pm_maps) == n
    assert sc.ks_maps[-1] == sc.textures.index("g.pgm") and sc.pr_maps[-1] == sc.pm_maps[-1] == sc.textures.index("orm.ppm")
    assert all(m == -1 for lst in (sc.ks_maps, sc.pr_maps, sc.pm_maps) for m in lst[:-1])
    assert np.array_equal(sc.texture_pixels[sc.pr_maps[-1]], rgb4) and np.array_equal(sc.texture_pixels[sc.ks_maps[-1]], g4)
    assert sc.ess_table is not None and sc.ess_table.shape == (17, 16)
    assert np.array_equal(bits(sc.ess_table[5]), bits(rt.generate_ess_lut(F(5) / F(16)))) and np.array_equal(bits(sc.ess_table), bits(rt.ess_table_rows(17)))
    # the zero-scalar rule: the file gives no Ks, Pr, Pm, the parser records zeros, the binding step sets them to one and regenerates the LUT
    m = np.asarray(sc.materials, np.float32)[-1]
    assert m[4:7].tolist() == [1, 1, 1] and m[12] == 1 and m[13] == 1
    assert np.array_equal(bits(m[16:32]), bits(rt.generate_ess_lut(1.0)))
    # ... spec_maps=False leaves the records as parsed, and so does NO_TEXTURES
    for kw in (dict(spec_maps=False), dict(textures=False)):
        sc0 = rt.Scene.from_obj(*write_quad(tmp_path, "map_Ks g.pgm\nmap_Pr orm.ppm\nmap_Pm orm.ppm\n"), **kw)
        m0 = np.asarray(sc0.materials, np.float32)[-1]
        assert m0[4:7].tolist() == [0, 0, 0] and m0[12] == 0 and m0[13] == 0, kw
        assert all(t == -1 for lst in (sc0.ks_maps, sc0.pr_maps, sc0.pm_maps) for t in lst) and sc0.ess_table is None
        assert sc0.material_ext[-1]["maps"]["Pr"] == "orm.ppm"              # (the parser's record of the statement stays)
    # a scalar the file does give is kept, and only the slot that has a map is touched
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "Ks 0.5 0.25 0\nPr 0.375\nmap_Pr g.pgm\nmap_Ks g.pgm\n"))
    m = np.asarray(sc.materials, np.float32)[-1]
    assert m[4:7].tolist() == [0.5, 0.25, 0] and m[12] == F(0.375) and m[13] == 0 and sc.pm_maps[-1] == -1
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Pm g.pgm\n"))
    m = np.asarray(sc.materials, np.float32)[-1]
    assert m[13] == 1 and m[12] == 0 and m[4:7].tolist() == [0, 0, 0] and sc.ess_table is None
    # a map whose image is missing is not bound, and the rule does not apply
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "map_Pr missing.ppm\n"))
    assert sc.pr_maps[-1] == -1 and np.asarray(sc.materials, np.float32)[-1][12] == 0
    # a file shared with `norm` under flip_y: the flipped normal map is a copy, the roughness slot reads the file's own bytes
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm orm.ppm\nmap_Pr orm.ppm\n"), flip_y=True)
    pr, nm = sc.pr_maps[-1], sc.normal_maps[-1]
    assert pr == sc.textures.index("orm.ppm") and nm == len(sc.textures) - 1 and nm != pr
    assert np.array_equal(sc.texture_pixels[pr], rgb4) and not np.array_equal(sc.texture_pixels[nm], rgb4)
    sc = rt.Scene.from_obj(*write_quad(tmp_path, "norm orm.ppm\nmap_Pr orm.ppm\n"))
    assert sc.pr_maps[-1] == sc.normal_maps[-1]                              # (nothing to change: one texture in both slots)


def test_golden_scenes_have_no_spec_maps(rt, golden_dir):
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    for lst in (sc.ks_maps, sc.pr_maps, sc.pm_maps):
        assert len(lst) == len(sc.materials) and all(m == -1 for m in lst)
    assert sc.ess_table is None and rt.Scene.cornell().pr_maps == [-1] * len(rt.Scene.cornell().materials)


# ------------------------------------------------------------------------------------------------
# the interface, the host code under the sanitizers
# ------------------------------------------------------------------------------------------------
def test_new_symbols_exist(rt):
    L = rt.lib
    names = ("rtx_set_ess_table", "rtx_debug_specular", "rtx_debug_ess", "rtxh_scene_spec_map")
    for name in names:
        assert getattr(L, name)
    assert (rt.MAP_KS, rt.MAP_PR, rt.MAP_PM) == (6, 8, 10) and rt.MAP_NORMAL == 4
    for f in ("set_ess_table", "specular", "ess"):
        assert callable(getattr(rt.Context, f))
    assert L.rtx_set_ess_table(None, None, 0) == -1 and L.rtx_debug_specular(None, None, 0, None) == -1 and L.rtx_debug_ess(None, 0, None, None, 0, None) == -1
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("enum { RTX_MAP_KS = 6, RTX_MAP_PR = 8, RTX_MAP_PM = 10 };", "enum { RTX_MAP_NORMAL = 4 };", "enum { RTX_MAP_KD = 0, RTX_MAP_OPACITY = 2 };", "SPECULAR MAPS",
                 "int  rtx_set_ess_table(rtx_ctx*, const float* table /* rows x 16 */, uint32_t rows);", "int  rtx_debug_specular(rtx_ctx*, const float* hits4, uint32_t n, float* out8);",
                 "int  rtx_debug_ess(rtx_ctx*, uint32_t material, const float* pr, const float* ndotv, uint32_t n, float* out);",
                 "Everything else stays the material's: Ks, Ke, Pr, Pm", "(unless SPECULAR MAPS, below)"):
        assert text in header, text
    host = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "#define RTXH_OBJ_NO_SPEC_MAPS   64u" in host and "rtxh_scene_spec_map(" in host
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in names:
        assert f" T {name}\n" in nm, name
    usage = subprocess.run([os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render"), "--help"], capture_output=True, text=True).stdout
    assert "--no-spec-maps" in usage


def test_specmap_host_header_under_asan_ubsan(tmp_path):
    """csrc/rtx_specmap_host.hpp as a stand-alone program (tests/sanitize/specmap_main.cpp: its own main, this header only) compiled with -fsanitize=address,undefined and run
    as a child process with nothing preloaded; its validation verdicts, rows, blended LUTs and zero-scalar results equal the twin's bit for bit (float32 * + - and floor are IEEE
    in both; the program is built without contraction)"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    exe = str(tmp_path / "san_specmap")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "royaltracer-dx_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "sanitize", "specmap_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    rng = np.random.default_rng(12)
    prs = np.concatenate([rng.uniform(0, 1, 30), [0.0, 1.0, 1.5, 100.0, -0.5, 0.5, 1.0 / 16.0, 65504.0]]).astype(np.float32)
    tabs = []                                                                # (rows, values, roughnesses)
    for rows in (2, 3, 17, 256):
        tabs.append((rows, rng.uniform(0.01, 1, rows * 16).astype(np.float32), prs))
    bad = rng.uniform(0.01, 1, 48).astype(np.float32); bad[47] = np.nan
    tabs.append((3, bad, prs[:2]))                                           # the LAST value is not finite: the check reads every one
    bad2 = bad.copy(); bad2[47] = 1.0; bad2[0] = -np.inf
    tabs.append((3, bad2, prs[:2]))
    tabs.append((1, np.ones(16, np.float32), prs[:2]))                       # too few rows
    tabs.append((257, np.ones(257 * 16, np.float32), prs[:2]))               # too many
    tabs.append((0, np.zeros(0, np.float32), prs[:2]))                       # NULL / 0: valid, clears
    recs = np.array([[0, 0, 0, 0, 0], [0, 0.5, 0, 0.25, 0], [1, 1, 1, 1, 1], [-0.0, 0, 0, -0.0, 0.5], [0, 0, 1e-30, 1e-30, 0]], np.float32)
    blob = struct.pack("<I", len(tabs))
    for rows, vals, pr in tabs:
        blob += struct.pack("<II", rows, len(vals)) + vals.tobytes() + struct.pack("<I", len(pr)) + pr.tobytes()
    blob += struct.pack("<I", len(recs)) + recs.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin")], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.split("\n")
    at = 0
    for rows, vals, pr in tabs:
        err = sr.table_error(vals if rows else None, rows)
        assert lines[at] == "V " + (err or "ok"), (rows, lines[at]); at += 1
        if err or not rows:
            continue
        r0, r1, wr = sr.ess_rows(pr, rows)
        for i, p in enumerate(pr):
            w = lines[at].split(); at += 1
            assert w[0] == "R" and int(w[1]) == r0[i] and int(w[2]) == r1[i] and bits(F(float.fromhex(w[3]))) == bits(wr[i]), (rows, p)
            w = lines[at].split(); at += 1
            got = np.array([float.fromhex(x) for x in w[1:]], np.float64).astype(np.float32)
            assert w[0] == "B" and np.array_equal(bits(got), bits(sr.blend_row(vals, p))), (rows, p)
    for rec in recs:
        w = lines[at].split(); at += 1
        want, ch = sr.zero_scalar_rule(rec)
        got = np.array([float.fromhex(x) for x in w[1:6]], np.float64).astype(np.float32)
        assert w[0] == "Z" and np.array_equal(bits(got), bits(want)) and tuple(int(x) for x in w[6:9]) == tuple(int(c) for c in ch), rec
    assert lines[at] == "done", r.stdout[-500:]

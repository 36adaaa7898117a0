"""Environment lighting without a GPU (include/rtx.h: rtx_set_environment): the properties of the definition itself on its numpy twin (tests/env_ref.py) — the octahedral
mapping, its solid-angle measure, the tables, the unbiasedness of the one-sample estimator pair —, the host layer's high-dynamic-range readers and latitude-longitude
conversion against the twin, the new symbols, and the host code under the sanitizers as a stand-alone program."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import env_ref as er

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def special_directions():
    """the axes, the fold seams (y = 0 plane, the diagonals of the lower pyramid) and signed zeros"""
    d = []
    for ax in range(3):
        for s in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]; v[ax] = s; d.append(v)
            for z in (0.0, -0.0):                                # the same axis with signed zeros elsewhere
                w = [z, z, z]; w[ax] = s; d.append(w)
    for a in np.linspace(0.0, 2.0 * math.pi, 16, endpoint=False):
        d.append([math.cos(a), 0.0, math.sin(a)])                # the seam between the upper face and the folded corners
        d.append([math.cos(a), -0.0, math.sin(a)])
    for t in (0.25, 0.5, 0.75):                                  # x = 0 and z = 0 in the lower hemisphere: where sgn decides the corner
        for s in (1.0, -1.0):
            d.append([0.0, -t, s * math.sqrt(1 - t * t)]); d.append([-0.0, -t, s * math.sqrt(1 - t * t)])
            d.append([s * math.sqrt(1 - t * t), -t, 0.0]); d.append([s * math.sqrt(1 - t * t), -t, -0.0])
    return np.array(d, np.float32)


def random_map(rng, n, zero_fraction=0.3):
    m = rng.uniform(0.0, 4.0, (n, n, 3)).astype(np.float32)
    m[rng.random((n, n)) < zero_fraction] = 0.0
    return m


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    m = np.eye(4)
    m[:3, :3] = q
    return m.T.reshape(16).astype(np.float32)                    # element (r, c) at [c * 4 + r]


# ------------------------------------------------------------------------------------------------
# (a) the mapping
# ------------------------------------------------------------------------------------------------
def test_encode_decode_round_trip():
    rng = np.random.default_rng(1)
    for n in (1, 8, 64, 2048):
        d = np.concatenate([unit(rng.normal(size=(4096, 3))), special_directions()])
        u, v, t, r3 = er.encode_env(d, n)
        assert (u >= 0).all() and (u <= 1).all() and (v >= 0).all() and (v <= 1).all() and (t >= 0).all() and (t < n * n).all()
        assert (r3 > 0.19).all() and (r3 <= 1.0 + 1e-6).all()
        q, r3d = er.decode_env(u, v)
        assert np.abs(q.astype(np.float64) - d).max() < 4e-6      # a few float32 roundings on components <= 1
        assert np.abs(r3d - r3).max() < 4e-6
        # ... and a texel's own centre comes back to the texel
        j, i = np.divmod(np.arange(n * n) if n <= 64 else rng.integers(0, n * n, 4096), n)
        qc, _ = er.decode_env((i + F(0.5)) / F(n), (j + F(0.5)) / F(n))
        assert np.array_equal(er.encode_env(qc, n)[2], j * n + i)
    # signed zeros: sgn(-0) = 1, so -0 and +0 components land in the same texel
    a = np.array([[0.0, -1.0, 0.0], [-0.0, -1.0, -0.0], [0.0, -0.5, 0.5], [-0.0, -0.5, 0.5]], np.float32)
    t = er.encode_env(a, 8)[2]
    assert t[0] == t[1] and t[2] == t[3]
    # the rotation: R^T (R q) = q up to rounding, and the identity is exact
    R = er.rot3(rotation(rng))
    q = unit(rng.normal(size=(256, 3)))
    assert np.abs(er.from_world(R, er.to_world(R, q)) - q).max() < 1e-6
    assert np.array_equal(bits(er.to_world(er.rot3(None), q)), bits(q))


# (b) the measure
def test_solid_angle_of_the_mapping():
    s = er.solid_angle_sum(2048)
    assert abs(s - 4.0 * math.pi) <= 1e-9 * 4.0 * math.pi, s
    x, y, z, w = er.grid_rows(512, np.arange(512))
    r3 = 4.0 / w
    assert r3.min() >= 0.192 and r3.max() <= 1.0 + 1e-12


# ------------------------------------------------------------------------------------------------
# (c) the tables
# ------------------------------------------------------------------------------------------------
def test_table_properties():
    rng = np.random.default_rng(2)
    for n in (1, 8, 64):
        m = random_map(rng, n) if n > 1 else np.ones((1, 1, 3), np.float32)
        if n > 1:
            m[n // 2] = 0.0                                       # a row without mass inside
            m[-1] = 0.0                                           # ... and the last one
            m[:, -1] = 0.0                                        # no row ends in a texel with mass
        tab = er.Tables(m)
        pmf = tab.texels[..., 3]
        assert abs(float(pmf.astype(np.float64).sum()) - 1.0) <= n * n * 2.0 ** -24
        zero = tab.w == 0
        assert np.array_equal(pmf == 0, zero)
        # both 2.0f rules
        rows = np.nonzero((~zero).any(axis=1))[0]
        assert (tab.marginal[rows[-1]:] == 2.0).all() and (tab.marginal[:rows[-1]] < 1.0 + 1e-6).all()
        for j in range(n):
            if j in rows:
                last = np.nonzero(~zero[j])[0][-1]
                assert (tab.conditional[j, last:] == 2.0).all() and (tab.conditional[j, :last] <= 1.0).all()
            else:
                assert (tab.conditional[j] == 2.0).all()
        assert (np.diff(tab.marginal) >= 0).all() and (np.diff(tab.conditional, axis=1) >= 0).all()
        # selection: 2^16 draws, xi = 1.0 and 0.0 among them, never a texel without mass
        xi_r = rng.random(1 << 16).astype(np.float32); xi_c = rng.random(1 << 16).astype(np.float32)
        xi_r[:4] = [1.0, 1.0, 0.0, 0.0]; xi_c[:4] = [1.0, 0.0, 1.0, 0.0]
        j = er.search(tab.marginal[None, :], xi_r)
        i = er.search(tab.conditional[j], xi_c)
        assert not zero[j, i].any()
        assert j[0] == rows[-1] and i[0] == np.nonzero(~zero[rows[-1]])[0][-1]      # xi = 1.0 lands on the last texel with mass
        # the frequencies follow the pmf (a chi-square-like bound on the busiest texels)
        cnt = np.bincount(j * n + i, minlength=n * n).reshape(n, n) / float(1 << 16)
        assert np.abs(cnt - pmf).max() < 6.0 * math.sqrt(float(pmf.max()) / (1 << 16)) + 1e-4
    # no mass at all: every entry 2.0f, total 0
    tab = er.Tables(np.zeros((8, 8, 3), np.float32))
    assert tab.total == 0.0 and (tab.marginal == 2.0).all() and (tab.conditional == 2.0).all() and (tab.texels == 0).all()
    # the scale is multiplied into the texels in float32, once
    m = random_map(rng, 8)
    assert np.array_equal(bits(er.Tables(m, 4.0).texels[..., :3]), bits(m * F(4.0)))
    assert np.array_equal(bits(er.Tables(m, 4.0).texels[..., 3]), bits(er.Tables(m).texels[..., 3]))      # a power of two changes no pmf bit


def test_tea_of_the_twin():
    """the twin's vectorised RandomFloat against a scalar replay of Common_v6.hlsl:119-138 in python integers (tests/test_env.py holds the device's draws to it)"""
    s0, s1 = np.array([1, 0xDEADBEEF, 0xFFFFFFFF], np.uint32), np.array([2, 0x12345678, 0xFFFFFFFF], np.uint32)
    v, a, b = er.tea_next(s0, s1)
    assert v.dtype == np.float32 and (v >= 0).all() and (v <= 1).all()
    # scalar replay in python integers
    for k in range(3):
        v0, v1, sm = int(s0[k]), int(s1[k]), 0
        for _ in range(4):
            sm = (sm + 0x9e3779b9) & 0xFFFFFFFF
            v0 = (v0 + ((((v1 << 4) + 0xA341316C) ^ (v1 + sm) ^ ((v1 >> 5) + 0xC8013EA4)) & 0xFFFFFFFF)) & 0xFFFFFFFF
            v1 = (v1 + ((((v0 << 4) + 0xAD90777D) ^ (v0 + sm) ^ ((v0 >> 5) + 0x7E95761E)) & 0xFFFFFFFF)) & 0xFFFFFFFF
        assert (int(a[k]), int(b[k])) == (v0, v1) and v[k] == F(np.float32(v0) * F(1.0 / 4294967296.0))


# ------------------------------------------------------------------------------------------------
# (d) the estimator pair is unbiased
# ------------------------------------------------------------------------------------------------
def sun_map():
    m = np.ones((8, 8, 3), np.float32)
    m[5, 2] = 1000.0
    return m


@pytest.mark.parametrize("name", ["constant", "sun"])
def test_estimator_pair_reproduces_the_irradiance(name):
    """environment NEE + BSDF miss on a Lambert plane facing +Y = rho E / pi, E by quadrature of the same map on a 4096^2 grid.  Tolerance: six times the std the twin
    measures on this input, over sqrt(n); the std is the one env_ref.py records for the GPU test (checked here to within a tenth)"""
    m, recorded = (np.ones((1, 1, 3), np.float32), er.CONST_STD) if name == "constant" else (sun_map(), er.SUN_STD)
    rho, n = 0.5, 1 << 18
    E = er.irradiance_up(m, 4096)[0]
    want = rho * E / math.pi
    x = er.estimator_pair(er.Tables(m), rho, n, 7)
    std = float(x.std())
    print(f"{name}: estimate {x.mean():.5f} against {want:.5f}, per-sample std {std:.4f} (recorded {recorded})")
    assert abs(std - recorded) <= 0.1 * recorded
    assert abs(float(x.mean()) - want) <= 6.0 * std / math.sqrt(n)
    if name == "constant":
        assert abs(want - rho) < 1e-6                             # E = pi for L = 1


# ------------------------------------------------------------------------------------------------
# (e) the readers
# ------------------------------------------------------------------------------------------------
def rgbe_decode(px):
    px = np.asarray(px, np.uint8)
    f = np.ldexp(np.float32(1.0), px[..., 3].astype(np.int32) - 136).astype(np.float32)
    out = px[..., :3].astype(np.float32) * f[..., None]
    out[px[..., 3] == 0] = 0.0
    return out


def rle_channel(row):
    """new-style run-length encoding of one channel of a scanline: runs of >= 3 equal bytes as (128 + count, value), the rest as literals of <= 128"""
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        run = 1
        while i + run < n and run < 127 and row[i + run] == row[i]:
            run += 1
        if run >= 3:
            out += bytes([128 + run, row[i]]); i += run
            continue
        j = i
        while j < n and j - i < 128:
            r = 1
            while j + r < n and r < 3 and row[j + r] == row[j]:
                r += 1
            if r >= 3:
                break
            j += 1
        out += bytes([j - i]) + bytes(row[i:j]); i = j
    return bytes(out)


def hdr_bytes(px, rle, header=b"#?RADIANCE\n# made by the test\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n", res=None):
    h, w = px.shape[:2]
    body = bytearray()
    for y in range(h):
        if rle:
            body += bytes([2, 2, w >> 8, w & 255])
            for c in range(4):
                body += rle_channel(px[y, :, c].tolist())
        else:
            body += px[y].tobytes()
    return header + (res if res is not None else b"-Y %d +X %d\n" % (h, w)) + bytes(body)


def pfm_bytes(img, little, magnitude=1.0):
    h, w = img.shape[:2]
    data = np.ascontiguousarray(img[::-1]).astype("<f4" if little else ">f4").tobytes()      # rows bottom-up
    return b"PF\n%d %d\n%s\n" % (w, h, (b"-" if little else b"") + repr(magnitude).encode()) + data


def test_hdr_and_pfm_readers(rt, tmp_path):
    rng = np.random.default_rng(3)
    px = rng.integers(0, 256, (7, 11, 4), dtype=np.uint8)
    px[..., 3] = rng.integers(100, 160, (7, 11))
    px[2, :, :] = px[2, 0, :]                                     # a row of one colour: long runs
    px[3, 4:9, 3] = 0                                             # exponent 0 is black
    wide = np.repeat(px, 30, axis=1)[:, :300]                     # runs and literals past 128, a width with a high byte
    for name, img, rle in (("flat.hdr", px, False), ("rle.hdr", px, True), ("wide.hdr", wide, True), ("narrow.hdr", px[:, :5], False)):
        (tmp_path / name).write_bytes(hdr_bytes(img, rle))
        got = rt.read_hdr_image(tmp_path / name)
        assert got.shape == img.shape[:2] + (3,) and np.array_equal(bits(got), bits(rgbe_decode(img))), name
    (tmp_path / "rgbe.hdr").write_bytes(hdr_bytes(px, True, header=b"#?RGBE\nFORMAT=32-bit_rle_rgbe\n\n"))
    assert np.array_equal(bits(rt.read_hdr_image(tmp_path / "rgbe.hdr")), bits(rgbe_decode(px)))
    img = rng.normal(size=(5, 9, 3)).astype(np.float32) * F(100.0)
    img[0, 0] = [0.0, -0.0, 1e-30]
    for name, little, mag in (("le.pfm", True, 1.0), ("be.pfm", False, 1.0), ("mag.pfm", True, 2.5)):
        (tmp_path / name).write_bytes(pfm_bytes(img, little, mag))
        assert np.array_equal(bits(rt.read_hdr_image(tmp_path / name)), bits(img)), name
    # truncated and corrupt files are refused
    good_rle, good_flat = hdr_bytes(px, True), hdr_bytes(px, False)
    over = bytearray(hdr_bytes(px[:, :9], True)); over[over.index(b"+X 9\n") + 5 + 4] = 128 + 100      # a run longer than the scanline
    bad = {"trunc_rle.hdr": good_rle[:-9], "trunc_flat.hdr": good_flat[:-5], "header_only.hdr": good_flat[:40], "overrun.hdr": bytes(over),
           "orient.hdr": hdr_bytes(px, False, res=b"+Y 7 +X 11\n"), "noformat.hdr": hdr_bytes(px, False, header=b"#?RADIANCE\n\n"),
           "xyze.hdr": hdr_bytes(px, False, header=b"#?RADIANCE\nFORMAT=32-bit_rle_xyze\n\n"), "width.hdr": hdr_bytes(wide, True).replace(b"+X 300", b"+X 299"),
           "zero.hdr": hdr_bytes(px, False, res=b"-Y 0 +X 11\n"), "huge.hdr": hdr_bytes(px, False, res=b"-Y 99999 +X 99999\n"),
           "trunc.pfm": pfm_bytes(img, True)[:-3], "grey.pfm": b"Pf\n9 5\n-1.0\n" + bytes(9 * 5 * 4), "scale0.pfm": b"PF\n9 5\n0\n" + bytes(9 * 5 * 12),
           "size.pfm": b"PF\n9\n-1.0\n" + bytes(9 * 5 * 12), "other.bin": bytes(64), "empty.hdr": b""}
    for name, data in bad.items():
        (tmp_path / name).write_bytes(data)
        with pytest.raises(rt.RtxError):
            rt.read_hdr_image(tmp_path / name)
    with pytest.raises(rt.RtxError):
        rt.read_hdr_image(tmp_path / "nothing.hdr")


# ------------------------------------------------------------------------------------------------
# (f) the latitude-longitude conversion
# ------------------------------------------------------------------------------------------------
def smooth_latlong(h, w):
    t = (np.arange(h) + 0.5) / h * math.pi
    p = (np.arange(w) + 0.5) / w * 2.0 * math.pi
    T, P = np.meshgrid(t, p, indexing="ij")
    x, y, z = np.sin(T) * np.sin(P), np.cos(T), -np.sin(T) * np.cos(P)
    return np.stack([1.0 + 0.5 * y + 0.25 * x, 0.6 + 0.3 * z * z, 0.8 + 0.2 * x * y], axis=-1).astype(np.float32)


# |octahedral integral / lat-long integral - 1| of the twin's conversion, measured by this test on the CPU (it prints them); the bounds are twice these
SMOOTH_ENERGY_ERR = 3.43e-4      # smooth image 96 x 48 -> 32 x 32 (S = 2)
SUN_ENERGY_ERR = 0.139           # one 1000 x pixel on a 96 x 48 image -> 32 x 32: about one nearest sub-position per pixel, so a single pixel is met by one or two of them
                                 # and its energy is kept to the tens of per cent only (96 x 192 -> 16 x 16, S = 6: 0.49); a sun wants a map at least as fine as its image


def test_latlong_conversion_against_the_twin(rt):
    rng = np.random.default_rng(4)
    for (h, w), n in (((48, 96), 32), ((37, 61), 8), ((64, 128), 5), ((16, 32), 1), ((9, 700), 16)):
        img = rng.uniform(0.0, 3.0, (h, w, 3)).astype(np.float32) if (h, w) != (48, 96) else smooth_latlong(h, w)
        got, want = rt.latlong_to_octahedral(img, n), er.latlong_to_octahedral(img, n)
        assert got.shape == (n, n, 3)
        # each side in double with its own libm: a sub-position within an ulp of a pixel boundary may fall either way, anything else agrees to the last bits
        close = np.abs(got.astype(np.float64) - want) <= 1e-6 * np.abs(want)
        assert close.mean() >= 0.999 and (close.all() or (h, w) != (48, 96)), (h, w, n, float(np.abs(got - want).max()))
    assert er.sub_samples(96, 32) == 2 and er.sub_samples(700, 16) == 16 and er.sub_samples(128, 5) == 13 and er.sub_samples(32, 1) == 16
    with pytest.raises(rt.RtxError):
        rt.latlong_to_octahedral(np.zeros((4, 8, 3), np.float32), 4096)
    # the directions: +Y is row 0, -Z the first column's left edge, +X a quarter turn on
    cols = np.zeros((4, 8, 3), np.float32)
    cols[0] = 1.0; cols[1:3, 2] = 2.0                              # +Y cap; phi in [pi / 2, 3 pi / 4): just past +X towards +Z
    o = er.latlong_to_octahedral(cols, 64)
    tab = er.Tables(o)
    assert tab.eval(np.array([[0.0, 1.0, 0.0]], np.float32))[0][0, 0] == 1.0
    assert tab.eval(unit([[math.sin(1.9), 0.0, -math.cos(1.9)]]))[0][0, 0] == 2.0
    assert tab.eval(unit([[math.sin(0.2), 0.0, -math.cos(0.2)]]))[0][0, 0] == 0.0


def test_latlong_conversion_conserves_energy():
    smooth = smooth_latlong(48, 96)
    sun = np.full((48, 96, 3), 0.01, np.float32)
    sun[14, 70] = 1000.0
    for img, err, name in ((smooth, SMOOTH_ENERGY_ERR, "smooth"), (sun, SUN_ENERGY_ERR, "sun")):
        o = er.latlong_to_octahedral(img, 32)
        a, b = er.latlong_integral(img), er.integrate(o, 1024)
        rel = float(np.abs(b / a - 1.0).max())
        print(f"{name}: lat-long {a}, octahedral {b}, relative error {rel:.3e} (recorded {err:.1e})")
        assert rel <= 2.0 * err


# ------------------------------------------------------------------------------------------------
# (g) the interface, (h) the host code under the sanitizers
# ------------------------------------------------------------------------------------------------
def test_new_symbols_exist(rt):
    L = rt.lib
    for name in ("rtx_set_environment", "rtx_debug_env_sample", "rtx_debug_env_eval", "rtx_debug_env_tables", "rtxh_read_hdr_image", "rtxh_env_from_latlong"):
        assert getattr(L, name)
    for name in ("set_environment", "env_sample", "env_eval", "env_tables"):
        assert callable(getattr(rt.Context, name))
    assert rt.ENV_HIDDEN == 1 and callable(rt.read_hdr_image) and callable(rt.latlong_to_octahedral)
    assert L.rtx_set_environment(None, None, 0, None, 1.0, 0) == -1 and L.rtx_debug_env_tables(None, None, None, None) == -1
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("#define RTX_ENV_HIDDEN 1u", "int  rtx_set_environment(", "int  rtx_debug_env_sample(", "int  rtx_debug_env_eval(", "int  rtx_debug_env_tables(",
                 "Lookup is NEAREST", "Bilinear lookup is not part of this"):
        assert text in header, text
    host = open(os.path.join(ROOT, "include", "rtx_host.h")).read()
    assert "rtxh_read_hdr_image(" in host and "rtxh_env_from_latlong(" in host
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in ("rtx_set_environment", "rtx_debug_env_sample", "rtx_debug_env_eval", "rtx_debug_env_tables", "rtxh_read_hdr_image", "rtxh_env_from_latlong"):
        assert f" T {name}\n" in nm, name


def test_environment_host_code_under_asan_ubsan(tmp_path):
    """the table builder, both readers and the conversion as a stand-alone program (tests/sanitize/env_main.cpp, its own main) compiled with -fsanitize=address,undefined and
    run as a child process on good, truncated and corrupt files; nothing sanitized is loaded into this interpreter"""
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    pk = os.path.join(ROOT, "royaltracer-dx_amd")
    exe = str(tmp_path / "san_env")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(pk, "csrc"), "-I" + os.path.join(pk, "host"),
           "-o", exe, os.path.join(ROOT, "tests", "sanitize", "env_main.cpp"), os.path.join(pk, "csrc", "rtx_env_host.cpp"), os.path.join(pk, "host", "ImageIO.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (6, 40, 4), dtype=np.uint8)
    img = rng.uniform(0, 5, (6, 12, 3)).astype(np.float32)
    over = bytearray(hdr_bytes(px, True)); over[over.index(b"+X 40\n") + 6 + 4] = 128 + 120
    files = {"a.hdr": hdr_bytes(px, True), "b.hdr": hdr_bytes(px, False), "c.pfm": pfm_bytes(img, True), "d.pfm": pfm_bytes(img, False),
             "t1.hdr": hdr_bytes(px, True)[:-7], "t2.hdr": hdr_bytes(px, False)[:-7], "t3.hdr": hdr_bytes(px, True)[:30], "over.hdr": bytes(over), "t4.pfm": pfm_bytes(img, True)[:-1],
             "t5.pfm": b"PF\n12 6\n", "junk.bin": bytes(range(200)), "lit.hdr": hdr_bytes(px, True)[:-3] + bytes([120])}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([exe] + [str(tmp_path / n) for n in files] + [str(tmp_path / "missing.hdr")], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = r.stdout.split("\n")
    assert lines[:4] == ["ok 40 6", "ok 40 6", "ok 12 6", "ok 12 6"] and sum(l.startswith("refused: ") for l in lines) == 9 and "done" in lines, r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]

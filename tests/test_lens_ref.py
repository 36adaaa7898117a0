"""The thin-lens camera (include/rtx.h, THIN LENS) without a GPU: the numpy twin tests/lens_ref.py is a thin lens — every ray passes through the point in focus, lens points fill
the aperture disk, an out-of-focus emitter spreads over the predicted circle of confusion — and the library exports the calls."""
import math
import os
import subprocess

import numpy as np
import pytest

import lens_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


class QuadScene:
    """quads with one material each, built by hand in the reference's data model (duck-typed like rt.Scene for Context.upload and Oracle.load).  materials: rows of
    (Kd3, Ke3); material 0 is the default one.  quads: (a, b, c, d, material): two triangles (a, b, c), (a, c, d), flat normals (cross(b - a, c - a) is the front)"""
    def __init__(self, materials, quads, view, proj):
        m = np.zeros((1 + len(materials), 32), np.float32)
        m[0, 0:4] = (1, 1, 1, 1); m[0, 12] = 1.0
        for i, (kd, ke) in enumerate(materials):
            m[1 + i, 0:4] = (*kd, 1); m[1 + i, 8:11] = ke; m[1 + i, 12] = 1.0
        self.materials = m
        v, idx, mid = [], [], []
        for a, b, c, d, mat in quads:
            base = len(v)
            v += [(*a, 0, 0, 0, 0), (*b, 0, 0, 0, 0), (*c, 0, 0, 0, 0), (*d, 0, 0, 0, 0)]
            idx += [base, base + 1, base + 2, base, base + 2, base + 3]; mid += [1 + mat] * 6
        self.meshes = [(np.array(v, np.float32), np.array(idx, np.uint32), np.array(mid, np.uint32))]
        self.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
        self.view, self.proj = view, proj
        self.quad_material = [q[4] for q in quads]              # triangle t belongs to quad t // 2

    def view_proj(self, aspect):
        return self.view, self.proj


def facing_quad(cx, cy, z, hx, hy, mat):
    """an axis-aligned quad in the plane z = const whose front faces +z (a camera looking down -z)"""
    return ((cx - hx, cy - hy, z), (cx + hx, cy - hy, z), (cx + hx, cy + hy, z), (cx - hx, cy + hy, z), mat)


def dist_to_line(p, o, d):
    """distance of the points p from the lines (o, d), float64"""
    p, o, d = (np.asarray(a, np.float64) for a in (p, o, d))
    return np.linalg.norm(np.cross(p - o, d), axis=1) / np.linalg.norm(d, axis=1)


@pytest.mark.parametrize("jitter", [0, lens_ref.JITTER])
def test_the_twin_is_a_thin_lens(rt, orc, jitter):
    """Every pixel of a 16 x 12 image of a random camera (lookAt + perspective), samples 1-8: the twin's ray (o', d') passes through P, and P is the pinhole ray's point at
    view-axis depth F.  BOUND, all distances evaluated in float64: 64 ulp (float32) of the largest coordinate magnitude among o, P and R — about 3 roundings in P, 4 in o', 4 in
    the normalised direction carried over |P - o'|, < 16 ulp in all, times 4."""
    W, H, R, F = 16, 12, 0.35, 4.5
    rng = np.random.default_rng(20)
    eye, ctr = rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
    view = rt.lookat(eye, ctr, (0.0, 1.0, 0.0))
    proj = rt.perspective_fov_rh(math.radians(50.0), W / H, 0.1, 1000.0)
    o = orc.Oracle(); o.set_camera(view, proj)
    Vi = orc.mat4_inverse(view)
    axis = np.asarray(Vi[8:11], np.float64)
    for s in range(1, 9):
        p = rt.Params(width=W, height=H, frame_seed=5, flags=jitter)
        rays, seeds, q = lens_ref.lens_rays(orc, o, p, s, view, R, F)
        assert not q["kept"].any()
        big = np.maximum(np.abs(q["o"]).max(1), np.abs(q["P"]).max(1)).clip(min=R)
        bound = 64.0 * np.spacing(big.astype(F32)).astype(np.float64)
        assert (dist_to_line(q["P"], rays[:, 0:3], rays[:, 4:7]) <= bound).all()
        assert (dist_to_line(q["P"], q["o"], q["d"]) <= bound).all()
        depth = np.abs((q["P"].astype(np.float64) - q["o"].astype(np.float64)) @ axis)
        assert (np.abs(depth - F) <= bound).all()
        assert np.allclose(np.linalg.norm(rays[:, 4:7].astype(np.float64), axis=1), 1.0, atol=1e-6)
        pin = o.primary_rays(p, s)
        assert np.array_equal(rays[:, 3], pin[:, 3]) and np.array_equal(rays[:, 7], pin[:, 7])      # tmin / tmax stay the camera rays'
        if jitter:
            assert not np.array_equal(seeds, lens_ref.seeds_without_lens(orc, W, H, s, 5, 0))


def test_lens_points_fill_the_disk(rt, orc):
    """65 536 (pixel, sample) draws (64 x 64 pixels, samples 1-16): |o' - o| <= R (1 + 2^-20), and the mean of |o' - o|^2 / R^2 — the mean of xi1 for a uniform disk — lies in
    0.5 +- 0.01 (5 sigma of 0.289 / sqrt(65536) is 0.0056).  The camera sits at the origin, where o' = o + ... adds to zero exactly: the bound is one on the lens-point arithmetic
    (two products and the table's sine and cosine, a few 2^-24 each), not on the rounding of o' to the float grid of a far-away eye, which would be ulp(|o|) / R."""
    W = H = 64
    R = 0.25
    view = rt.lookat((0.0, 0.0, 0.0), (0.3, -0.2, -1.0), (0.0, 1.0, 0.0))
    proj = rt.perspective_fov_rh(math.radians(60.0), 1.0, 0.1, 1000.0)
    o = orc.Oracle(); o.set_camera(view, proj)
    r2 = []
    for s in range(1, 17):
        rays, _, q = lens_ref.lens_rays(orc, o, rt.Params(width=W, height=H, frame_seed=1, flags=0), s, view, R, 3.0)
        assert not np.abs(q["o"]).any()
        d = (rays[:, 0:3].astype(np.float64) - q["o"].astype(np.float64))
        r2.append((d * d).sum(1))
    r2 = np.concatenate(r2)
    assert len(r2) == 65536
    assert (np.sqrt(r2) <= R * (1.0 + 2.0 ** -20)).all()
    assert abs((r2 / (R * R)).mean() - 0.5) <= 0.01


def test_circle_of_confusion(rt, orc):
    """A 2 x 2-pixel-sized emissive quad at view depth z in front of black geometry, focus F != z, 64 samples: the pixels in which some twin ray's closest hit (the oracle's
    tracer) is the emitter lie within the predicted circle of confusion, R |z - F| / z * (H / 2) / (F tan(fovy / 2)) pixels, + the quad's half-size + 1, of the quad's pinhole
    image — and reach that radius minus 2."""
    W, H, fovy = 32, 24, math.radians(60.0)
    z, F, R = 1.0, 3.0, 0.5774
    px_per_tan = (H / 2) / math.tan(fovy / 2)
    radius = R * abs(z - F) / z * (H / 2) / (F * math.tan(fovy / 2))
    assert 6.0 <= radius <= 10.0
    half = z / px_per_tan                                           # one pixel at depth z
    view = rt.lookat((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    proj = rt.perspective_fov_rh(fovy, W / H, 0.1, 1000.0)
    sc = QuadScene([((0, 0, 0), (4.0, 2.0, 1.0)), ((0, 0, 0), (0, 0, 0))], [facing_quad(0, 0, -z, half, half, 0), facing_quad(0, 0, -10.0, 30.0, 30.0, 1)], view, proj)
    o = orc.Oracle().load(sc, W / H)
    p = rt.Params(width=W, height=H, frame_seed=3, flags=0)
    pin = o.trace_closest(o.primary_rays(p, 1), 0)[:, 3].view(np.uint32)
    pin_lit = np.flatnonzero(pin < 2)
    assert len(pin_lit) and all(abs(i % W - W / 2) <= 1 and abs(i // W - H / 2) <= 1 for i in pin_lit)      # the quad's pinhole image: at the image centre
    lit = np.zeros(W * H, bool)
    for s in range(1, 65):
        rays, _, _ = lens_ref.lens_rays(orc, o, p, s, view, R, F)
        lit |= o.trace_closest(rays, 0)[:, 3].view(np.uint32) < 2                                             # triangles 0 and 1 are the emitter
    idx = np.flatnonzero(lit)
    dist = np.hypot(idx % W - W / 2, idx // W - H / 2)
    assert len(idx) > len(pin_lit)
    assert dist.max() <= radius + 1.0 + 1.0
    assert dist.max() >= radius - 2.0


def test_ctypes_layout_and_exports(rt):
    """sizeof(Lens) == 16, the three symbols are exported and bound, the header declares them; the library loads without a GPU"""
    import ctypes as C
    assert C.sizeof(rt.Lens) == 16 and [n for n, _ in rt.Lens._fields_] == ["aperture_radius", "focus_distance", "reserved"]
    for name in ("rtx_set_lens", "rtx_focus_distance_at", "rtx_debug_primary_seeds"):
        assert getattr(rt.lib, name)
    for name in ("set_lens", "focus_distance_at", "primary_seeds"):
        assert callable(getattr(rt.Context, name))
    assert rt.lib.rtx_set_lens(None, None) == -1 and rt.lib.rtx_focus_distance_at(None, 1, 1, 0, 0, None) == -1       # RTX_ERR_INVALID: no context
    header = open(os.path.join(ROOT, "include", "rtx.h")).read()
    for text in ("typedef struct rtx_lens", "int  rtx_set_lens(", "int  rtx_focus_distance_at(", "int  rtx_debug_primary_seeds(", "THIN LENS"):
        assert text in header, text
    nm = subprocess.run(["nm", "-DC", "--defined-only", os.path.join(ROOT, "royaltracer-dx_amd", "librtx_hip.so")], capture_output=True, text=True).stdout
    for name in ("rtx_set_lens", "rtx_focus_distance_at", "rtx_debug_primary_seeds"):
        assert f" T {name}\n" in nm, name
    usage = subprocess.run([os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render"), "--help"], capture_output=True, text=True).stdout
    assert "--aperture" in usage and "--focus-pixel" in usage

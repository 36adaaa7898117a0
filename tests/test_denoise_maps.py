"""rtx_denoise's two opt-in guide extensions on the GPU (include/rtx.h, DENOISING: MAP GUIDES) against the float32 twin of tests/denoise_maps_ref.py: the map guides and the
denoised image bit for bit in all channels under every staging choice, the pixel counts exact, u1 untouched; the stated consequences; errors; the upper layers.
The world is that of tests/test_normalmap.py (about 200 triangles) at 64 x 48, 37 x 19 and 8 x 8: every tile of 8 x 8 is partial, and from level 3 on nearly every coarse tap
lies outside the image.  That the inputs are not vacuous is shown on the CPU (tests/test_denoise_maps_ref.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import denoise_maps_ref as mr
import test_denoise_ref as ref
from denoise_maps_ref import F, KW, NOGEO, SIZES
from test_normalmap import H, PT, W, context

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4
VARIANTS = ("KD", "KD+CUT")
LDS_STEPS = (4, 0, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_image(a, b, what):
    d = bits(a) != bits(b)
    assert not d.any(), f"{what}: {int(d.any(-1).sum())} pixels differ (first at {tuple(np.argwhere(d.any(-1))[0])}; w differs in {int(d[..., 3].sum())})"


def device_guides(rt, c, tab, w, h):
    """the device's guide record and the twin's map guides from the device's own guide rays and closest hits"""
    rays = c.primary_rays(rt.Params(width=w, height=h, flags=0))
    hits = c.trace_closest(rays)
    g = c.denoise_guides(w, h)
    return g, mr.map_guides(tab, rays, hits, g)


@pytest.fixture(scope="module")
def ctxs(rt):
    """one context per variant, shared by the tests that only render and denoise"""
    cs = {name: context(rt, [], mr.variant(name)) for name in VARIANTS}
    yield cs
    for c in cs.values():
        c.close()


@functools.lru_cache(maxsize=None)
def tables(name):
    return mr.Tables(mr.variant(name))


# ---- 1: the map guides ----
@pytest.mark.parametrize("gpu_build", [0, 1])
@pytest.mark.parametrize("name", VARIANTS)
def test_map_guides_equal_the_twin(rt, name, gpu_build):
    c = context(rt, [("OPT_GPU_BUILD", gpu_build)], mr.variant(name))
    try:
        for w, h in SIZES:
            g0 = c.denoise_guides(w, h)
            g, want = device_guides(rt, c, tables(name), w, h)
            got = c.denoise_map_guides(w, h)
            d = (bits(got) != bits(want)).any(-1)
            assert not d.any(), f"{name}, {w} x {h}: {int(d.sum())} pixels differ (first at {tuple(np.argwhere(d)[0])})"
            assert np.array_equal(bits(c.denoise_guides(w, h)), bits(g0)), "rtx_debug_denoise_guides is unchanged by the new entry"
            geo = bits(g)[..., 3] != NOGEO
            assert (got[~geo] == np.array([1, 1, 1, 0, 0, 0, 0, 0], F)).all() and not got[..., 3].any() and not got[..., 7].any()
        if name == "KD":                                                    # without cut-outs the oracle's first hits give the same record
            assert np.array_equal(bits(c.denoise_map_guides(W, H)), bits(mr.oracle_inputs("KD")[3]))
    finally:
        c.close()


# ---- 2: parity ----
def flags_kw(flags):
    return dict(albedo=bool(flags & mr.ALBEDO), mapped_normals=bool(flags & mr.MAPPED_NORMALS))


def check(rt, c, a, g, mg, levels, flags, what, lds_steps=LDS_STEPS):
    """denoise(levels, flags) == the twin under every staging choice; counts exact; returns the image"""
    h, w = a.shape[:2]
    e, nf = mr.emulate_maps(a, g, mg, levels, flags, **KW) if flags else ref.emulate(a, g, levels, **KW)
    d = None
    try:
        for lds in lds_steps:
            c.set_option(rt.OPT_DENOISE_LDS_STEP, lds)
            res = c.denoise(w, h, levels, **KW, **flags_kw(flags))
            d = c.read_denoised()
            same_image(d, e, f"{what}, flags {flags}, levels {levels}, LDS up to step {lds}")
            assert (res.levels, res.pixels_filtered, res.pixels_passed) == (levels, nf, w * h - nf), what
    finally:
        c.set_option(rt.OPT_DENOISE_LDS_STEP, 4)
    return d


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", VARIANTS)
def test_denoised_image_matches_the_twin(rt, ctxs, name, size):
    c = ctxs[name]
    w, h = size
    c.clear(w, h)
    c.render(rt.Params(**dict(PT, width=w, height=h)))
    a = c.read_accum()
    g, mg = device_guides(rt, c, tables(name), w, h)
    plain = check(rt, c, a, g, mg, 5, 0, name)
    for flags in (1, 2, 3):
        for levels in (1, 3, 5):
            d = check(rt, c, a, g, mg, levels, flags, name)
        if (w, h) == (W, H):
            assert not np.array_equal(bits(d), bits(plain)), f"flags {flags} changes the image of this frame"
    same_image(c.read_accum(), a, "u1 after the denoise")


# ---- 3: the consequences rtx.h states ----
@pytest.mark.parametrize("scene", ["unmapped", "flat_mapped"])
def test_mapped_normals_without_relief_is_the_plain_filter(rt, scene):
    c = context(rt, [], getattr(mr.world(), scene))
    try:
        c.clear(W, H); c.render(rt.Params(**PT))
        g = c.denoise_guides(W, H)
        assert np.array_equal(bits(c.denoise_map_guides(W, H))[..., 4:7], bits(g)[..., 4:7]), "nm == n to the bit"
        for lds in LDS_STEPS:
            c.set_option(rt.OPT_DENOISE_LDS_STEP, lds)
            c.denoise(W, H, 5, **KW); d0 = c.read_denoised()
            c.denoise(W, H, 5, mapped_normals=True, **KW)
            same_image(c.read_denoised(), d0, f"{scene}: flag 2 against flag 0, LDS up to step {lds}")
    finally:
        c.close()


def test_pass_through_pixels_of_a_caller_owned_u1(rt, ctxs):
    """flags 3: a pixel that is not FILTERABLE comes out as it went in, to the bit — pixels without samples whose xyz is not zero, one of them a NaN, and the pixels that are
    not filterable by geometry: the emitter seen directly and the misses through the holes of the cut-out walls"""
    import torch
    c = ctxs["KD+CUT"]
    c.clear(W, H); c.render(rt.Params(**PT))
    a = np.array(c.read_accum(), F, copy=True)
    g, mg = device_guides(rt, c, tables("KD+CUT"), W, H)
    geo = bits(g)[..., 3] != NOGEO
    assert (~geo).any() and (a[~geo][:, :3] > 0).any(), "the emitter is seen directly"
    a[25:35, 10:30, 3] = 0                                          # no samples, xyz kept: nonzero
    ny, nx = (int(v) for v in np.argwhere(geo[25:35, 10:30])[0] + (25, 10))
    a[ny, nx, 0] = np.nan
    a[~geo, 0] *= F(3)                                              # (a colour the filter would not leave alone if it touched it)
    assert geo[25:35, 10:30].sum() >= 100 and (a[25:35, 10:30, :3] != 0).any()
    passes = ~(geo & (a[..., 3] > 0))
    with np.errstate(invalid="ignore"):
        mean = a[..., :3] / np.maximum(a[..., 3:], F(1))
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    c.bind_accum(t.data_ptr(), t.numel() * 4)
    try:
        c.clear(W, H)
        t.copy_(torch.from_numpy(a)); torch.cuda.synchronize()
        for levels in (1, 5):
            d = check(rt, c, a, g, mg, levels, 3, "caller-owned u1")
            assert np.array_equal(bits(d[..., :3])[passes], bits(mean)[passes]) and (d[..., 3] == 1).all()
        assert np.isnan(d[ny, nx, 0]) and np.isfinite(d[geo & ~passes]).all(), "the NaN stays where it is: no tap reads a pass-through pixel"
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(a)), "u1 after the denoise"
    finally:
        c.bind_accum(None, 0)
        c.clear(W, H)


# ---- 4: what the extension is for, on the device ----
def test_albedo_detail_survives_on_the_device(rt, ctxs):
    """u1 = A * L from the DEVICE's A: flag 1 returns it within relative 2^-18 at every pixel; flag 0 moves the pixels tests/test_denoise_maps_ref.py printed by more than 5 %"""
    import torch
    c = ctxs["KD"]
    mg = c.denoise_map_guides(W, H)
    a = mr.synthetic_accum(mg)
    moved, _ = mr.moved_under_flag0("KD")
    assert moved.any()
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    c.bind_accum(t.data_ptr(), t.numel() * 4)
    try:
        c.clear(W, H)
        t.copy_(torch.from_numpy(a)); torch.cuda.synchronize()
        c.denoise(W, H, 5, albedo=True, **KW)
        e1 = mr.rel_err(c.read_denoised(), a)
        print(f"flag 1: largest relative error {e1.max():.3e} (bound {mr.REL:.3e})")
        assert (e1 <= mr.REL).all()
        c.denoise(W, H, 5, **KW)
        e0 = mr.rel_err(c.read_denoised(), a)
        print(f"flag 0: {int((e0[moved] > 0.05).sum())} of the twin's {int(moved.sum())} pixels move by more than 5 %")
        assert (e0[moved] > 0.05).all()
    finally:
        c.bind_accum(None, 0)
        c.clear(W, H)


# ---- 5: errors ----
def test_errors(rt, ctxs):
    c = ctxs["KD"]
    c.clear(W, H); c.render(rt.Params(**PT))
    a = c.read_accum()
    c.denoise(W, H, 3, albedo=True, **KW)
    d0 = c.read_denoised()
    for words in ((4, 0, 0, 0), (7, 0, 0, 0), (8, 0, 0, 0), (0x80000001, 0, 0, 0), (1, 1, 0, 0), (0, 0, 1, 0), (3, 0, 0, 1)):
        dp = rt.DenoiseParams(3, 5, 0.5, 0.0625, (C.c_uint32 * 4)(*words))
        assert rt.lib.rtx_denoise(c._h, W, H, C.byref(dp), None) == INVALID, words
        assert rt.lib.rtx_last_error(c._h)
    same_image(c.read_denoised(), d0, "the denoised image after the invalid calls"); same_image(c.read_accum(), a, "u1 after the invalid calls")
    buf = np.zeros((8, 8, 8), F)
    assert rt.lib.rtx_debug_denoise_map_guides(c._h, 8, 8, None) == INVALID and rt.lib.rtx_debug_denoise_map_guides(c._h, 0, 8, buf.ctypes.data_as(C.c_void_p)) == INVALID
    n = rt.Context(0)
    try:
        sc = mr.world().plain
        call = lambda: rt.lib.rtx_debug_denoise_map_guides(n._h, 8, 8, buf.ctypes.data_as(C.c_void_p))
        assert call() == STATE, "before commit"
        n.set_materials(sc.materials)
        for v, i, m in sc.meshes:
            n.add_mesh(v, i, m)
        for mesh, o2w in sc.instances:
            n.add_instance(mesh, o2w)
        n.commit()
        assert call() == STATE, "before the camera"
        n.set_camera(*sc.view_proj(W / H))
        assert call() == rt.RTX_OK
        assert (buf[..., 0:3] >= mr.FLOOR).all(), "a scene without any map: A = max(m.Kd, 2^-6)"
    finally:
        n.close()


# ---- 6: the upper layers ----
def test_renderer_facade_passes_the_flags(rt, cornell):
    """Renderer.read_denoised(albedo=True) on the Cornell box (no maps: A = max(m.Kd, 2^-6), constant per material) is the twin's image of the renderer's own guides"""
    r = rt.Renderer(W, H, "denoise maps")
    view = rt.Context.__new__(rt.Context)                          # a borrowed view of the renderer's context, for its guides: never closed from here
    view._h, view.width, view.height = None, W, H
    try:
        r.set_scene(cornell)
        r.params.spp, r.params.flags, r.params.max_bounces, r.params.nee_samples = 4, 1, 8, 1
        r.on_init(); r.on_update(); r.on_render()
        a = r.read_accum()
        d0, d1 = r.read_denoised(**KW), r.read_denoised(albedo=True, mapped_normals=True, **KW)
        view._h = rt.lib.rtxh_renderer_context(r._h)
        g, mg = view.denoise_guides(W, H), view.denoise_map_guides(W, H)
        same_image(d0, ref.emulate(a, g, 5, **KW)[0], "Renderer.read_denoised()")
        same_image(d1, mr.emulate_maps(a, g, mg, 5, 3, **KW)[0], "Renderer.read_denoised(albedo=True, mapped_normals=True)")
        assert not np.array_equal(bits(d1), bits(d0))
        same_image(r.read_accum(), a, "u1 after Renderer.read_denoised")
    finally:
        view._h = None
        r.close()


def test_cli(rt, tmp_path):
    """rtx_render --denoise --denoise-albedo --denoise-mapped-normals on an OBJ with a map_Kd and a norm writes an image that differs from the plain --denoise one and equals a
    Context doing the same; either flag without --denoise is a usage error"""
    from test_cutout_ref import write_card
    from test_denoise import read_exr_rgb
    rng = np.random.default_rng(12)
    (tmp_path / "k.ppm").write_bytes(b"P6 7 6 255\n" + rng.integers(0, 256, (6, 7, 3), dtype=np.uint8).tobytes())
    (tmp_path / "n.ppm").write_bytes(b"P6 5 4 255\n" + rng.integers(0, 256, (4, 5, 3), dtype=np.uint8).tobytes())
    files, mtl = write_card(tmp_path, "map_Kd k.ppm\nnorm n.ppm\n")
    exe = os.path.join(graft.PKG_DIR, "rtx_render")

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run([exe, "--obj", files[0], "--mtl", mtl, "--w", str(W), "--h", str(H), "--spp", "4", "--out", out] + list(extra), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out)
    plain = cli("p.exr", "--denoise")
    both = cli("b.exr", "--denoise", "--denoise-albedo", "--denoise-mapped-normals")
    assert both.sum() > 0 and not np.array_equal(bits(both), bits(plain))
    c = rt.Context(0)
    try:
        c.upload(rt.Scene.from_obj(files, mtl), W / H); c.clear(W, H)
        c.render(rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0))
        c.denoise(W, H, albedo=True, mapped_normals=True)
        assert np.array_equal(bits(both), bits(c.read_denoised()[..., :3]))
    finally:
        c.close()
    for flag in ("--denoise-albedo", "--denoise-mapped-normals"):
        r = subprocess.run([exe, "--scene", "cornell", flag], capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--denoise" in r.stderr, (flag, r.returncode, r.stderr[-300:])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise-albedo" in r.stdout and "--denoise-mapped-normals" in r.stdout

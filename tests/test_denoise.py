"""rtx_denoise on the GPU against the float32 emulation of tests/test_denoise_ref.py (guides from the oracle's first hit + the filter of include/rtx.h): the guides and the
denoised image bit for bit in all channels, the pixel counts exact, u1 untouched.  Cornell box at 100 x 50, 37 x 19 and 8 x 8 (every tile partial; from level 3 on every
coarse tap but the centre lies outside), on the fused tiny-scene context and on the general BVH one, every level through the LDS-staged and the direct kernel.  The inputs
are shown non-vacuous on the CPU (test_denoise_ref.py::test_inputs_are_not_vacuous)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import test_adaptive_ref as aref
import test_denoise_ref as ref
from test_denoise_ref import BASE, SPP, SIGMA_COLOR, SIGMA_PLANE, NORMAL_POWER_LOG2, W, H, ASPECT, F, NOGEO
from test_deform import ArrayScene, place

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4
KW = dict(sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE, normal_power_log2=NORMAL_POWER_LOG2)
PATHS = ("fused", "general")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_image(a, b, what):
    d = bits(a) != bits(b)
    assert not d.any(), f"{what}: {int(d.any(-1).sum())} pixels differ (first at {tuple(np.argwhere(d.any(-1))[0])}; w differs in {int(d[..., 3].sum())})"


@pytest.fixture(scope="module")
def fused(rt, cornell):
    """the default context of a tiny scene: the guides through the plane / edge pre-test"""
    c = rt.Context(0)
    c.upload(cornell, ASPECT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def general(rt, cornell):
    """the same box on the general BVH path: the guides through the wide tree"""
    c = rt.Context(0)
    c.set_option(rt.OPT_SMALL_SCENE, 0)
    c.upload(cornell, ASPECT)
    yield c
    c.close()


@pytest.fixture
def ctx(request, fused, general):
    return fused if request.param == "fused" else general


def render(rt, c, flags, w=W, h=H):
    c.clear(w, h)
    c.render(rt.Params(**dict(BASE, width=w, height=h, spp=SPP, flags=flags)))
    return c.read_accum()


def check(c, a, g, levels, what, lds_steps=(4, 0, 2)):
    """denoise(levels) == emulate(a, g) under every staging choice; counts exact; returns the image"""
    h, w = a.shape[:2]
    e, nf = ref.emulate(a, g, levels)
    rt = graft.load_package()
    d = None
    try:
        for lds in lds_steps:
            c.set_option(rt.OPT_DENOISE_LDS_STEP, lds)
            res = c.denoise(w, h, levels, **KW)
            d = c.read_denoised()
            same_image(d, e, f"{what}, levels {levels}, LDS up to step {lds}")
            assert (res.levels, res.pixels_filtered, res.pixels_passed) == (levels, nf, w * h - nf), what
    finally:
        c.set_option(rt.OPT_DENOISE_LDS_STEP, 4)
    return d


# ---- guides ----
@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_guides_equal_the_oracles_first_hit(ctx):
    for w, h in ((W, H), (37, 19), (8, 8)):
        g = ctx.denoise_guides(w, h)
        assert np.array_equal(bits(g), bits(ref.cornell_guides(w, h))), f"{w} x {h}: {int((bits(g) != bits(ref.cornell_guides(w, h))).any(-1).sum())} pixels differ"
    m = bits(ctx.denoise_guides(W, H))[..., 3]
    assert (m == NOGEO).any() and (m != NOGEO).any()


@pytest.mark.parametrize("small", [1, 0])
def test_guides_do_not_see_a_hidden_instance(rt, small):
    """Cornell box + a 12-triangle box in front of the back wall: hidden, the guides are the plain Cornell box's; shown, the scene's with the box"""
    cb = rt.Scene.cornell()
    base = sum(len(m) for _, _, m in cb.meshes)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    bv = np.zeros((8, 7), np.float32); bv[:, :3] = corners; bv[:, 6] = float(base)
    bi = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3], np.uint32)
    mats = np.asarray(cb.materials, np.float32)
    meshes = list(cb.meshes) + [(bv, bi, np.full(len(bi), int(np.argmin(mats[:, 8:11].sum(1))), np.uint32))]
    insts = list(cb.instances) + [(1, place(0.42, 0.31, 0.37, 0.2, 0.25, 0.2))]
    full = ArrayScene(mats, meshes, insts, cb.view_proj, -0.2, 1.2)
    plain = ArrayScene(mats, meshes, insts[:1], cb.view_proj, -0.2, 1.2)
    g_full, g_plain = ref.guides_of(full, W, H, ASPECT), ref.guides_of(plain, W, H, ASPECT)
    assert not np.array_equal(bits(g_full), bits(g_plain)), "the box is in view"
    c = rt.Context(0)
    try:
        c.set_option(rt.OPT_SMALL_SCENE, small)
        c.upload(full, ASPECT)
        assert np.array_equal(bits(c.denoise_guides(W, H)), bits(g_full))
        c.set_instance_visible(1, False); c.commit()
        assert np.array_equal(bits(c.denoise_guides(W, H)), bits(g_plain))
        # ... and so does the filter: the denoised image of the hidden state is the emulation with the plain box's guides
        a = render(rt, c, 1)
        check(c, a, g_plain, 3, f"box hidden, small scene {small}", lds_steps=(4,))
    finally:
        c.close()


# ---- parity ----
@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_denoised_image_matches_the_emulation(rt, ctx, flags):
    a = render(rt, ctx, flags)
    if flags == 1:
        same_image(a, ref.oracle_accum(1), "the accumulation is the oracle's")
    for levels in (1, 3, 5):
        check(ctx, a, ref.cornell_guides(), levels, f"flags {flags}")
    same_image(ctx.read_accum(), a, "u1 after the denoise")


@pytest.mark.parametrize("size", [(37, 19), (8, 8)])
@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_small_frames(rt, ctx, size):
    w, h = size
    a = render(rt, ctx, 1, w, h)
    g = ref.cornell_guides(w, h)
    assert ((bits(g)[..., 3] != NOGEO) & (a[..., 3] > 0)).sum() >= 40
    for levels in (1, 3, 5):
        check(ctx, a, g, levels, f"{w} x {h}")
    same_image(ctx.read_accum(), a, "u1 after the denoise")


@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_after_adaptive_sampling(rt, ctx):
    ctx.clear(W, H)
    ctx.render_adaptive(rt.Params(**dict(aref.BASE, flags=1, tile_size=16)), aref.MIN_SPP, aref.STEP_SPP, aref.MAX_SPP, aref.THRESHOLD)
    a = ctx.read_accum()
    assert len(np.unique(a[..., 3])) > 1, "adaptive sampling left non-uniform counts"
    check(ctx, a, ref.cornell_guides(), 3, "after render_adaptive")
    same_image(ctx.read_accum(), a, "u1 after the denoise")


@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_caller_owned_u1_with_cases_the_renderer_never_produces(rt, ctx):
    import torch
    g = ref.cornell_guides()
    a = np.array(ref.oracle_accum(1), F, copy=True)
    geo = bits(g)[..., 3] != NOGEO
    a[10:20, 30:50] = 0                                            # a block without samples, inside the box
    a[25] = a[25] * F(250)                                         # one row with count 1000
    assert (a[25, :, 3] == 1000).all() and geo[10:20, 30:50].any() and geo[25].any()
    hy, hx = 35, 50                                                # a filterable pixel a million times too bright: wc == 0 for everything but itself
    assert geo[hy, hx] and a[hy, hx, 3] > 0
    a[hy, hx, :3] = F(1e6) * a[hy, hx, 3]
    t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    ctx.bind_accum(t.data_ptr(), t.numel() * 4)
    try:
        ctx.clear(W, H)
        t.copy_(torch.from_numpy(a)); torch.cuda.synchronize()
        same_image(ctx.read_accum(), a, "the bound tensor")
        for levels in (1, 3):
            d = check(ctx, a, g, levels, "caller-owned u1")
        assert (d[10:20, 30:50] == np.array([0, 0, 0, 1], F)).all(), "pixels without samples pass through as (0, 0, 0, 1)"
        assert d[hy, hx, 0] > 1e5, "the outlier keeps its colour: no tap but the centre has weight"
        # ... and they changed no neighbour: the same image as when those pixels are misses
        g2 = np.array(g, F, copy=True); g2[10:20, 30:50] = 0; bits(g2)[10:20, 30:50, 3] = NOGEO
        same_image(d, ref.emulate(a, g2, 3)[0], "sample-less pixels count for no neighbour")
        torch.cuda.synchronize()
        same_image(t.cpu().numpy(), a, "u1 after the denoise")
    finally:
        ctx.bind_accum(None, 0)
        ctx.clear(W, H)


# ---- defaults, sRGB8 ----
def default_sigma_plane(scene):
    """include/rtx.h: 2^-6 * the largest extent of the box of every instance's vertices, world_k = ((v.x m[k] + v.y m[4+k]) + v.z m[8+k]) + m[12+k] in float32"""
    lo, hi = np.full(3, np.inf, F), np.full(3, -np.inf, F)
    for mesh, m in scene.instances:
        v, m = np.asarray(scene.meshes[mesh][0], F)[:, :3], np.asarray(m, F)
        for k in range(3):
            wk = ((v[:, 0] * m[k] + v[:, 1] * m[4 + k]) + v[:, 2] * m[8 + k]) + m[12 + k]
            assert wk.dtype == F
            lo[k], hi[k] = min(lo[k], wk.min()), max(hi[k], wk.max())
    return F(0.015625) * (hi - lo).max()


@pytest.mark.parametrize("ctx", PATHS, indirect=True)
def test_defaults(rt, ctx, cornell):
    a = render(rt, ctx, 1)
    sp = default_sigma_plane(cornell)
    lo, hi = cornell.bounds()
    assert sp == F(2 ** -6) * F((hi - lo).max()), "on this scene Scene.bounds() gives the same box"
    res = ctx.denoise(W, H)
    d0 = ctx.read_denoised()
    assert res.levels == 5
    ctx.denoise(W, H, levels=5, normal_power_log2=5, sigma_color=0.5, sigma_plane=float(sp))
    same_image(ctx.read_denoised(), d0, "all zeros vs the explicit defaults")
    same_image(d0, ref.emulate(a, ref.cornell_guides(), 5, 0.5, sp, 5)[0], "the defaults vs the emulation")
    ctx.denoise(W, H, sigma_plane=float(sp) * 0.25)
    assert not np.array_equal(bits(ctx.read_denoised()), bits(d0)), "sigma_plane matters on this frame"


def test_srgb8_of_the_denoised_image(rt, orc, fused):
    render(rt, fused, 1)
    fused.denoise(W, H, 3, **KW)
    assert np.array_equal(fused.read_denoised_srgb8(), orc.srgb8(fused.read_denoised()))
    assert not np.array_equal(fused.read_denoised_srgb8(), fused.read_srgb8())


# ---- errors ----
def test_errors_leave_both_images_untouched(rt, cornell):
    c = rt.Context(0)
    buf = np.zeros((H, W, 4), F)
    buf8 = np.zeros((H, W, 4), np.uint8)

    def rc(w=W, h=H, levels=3, npow=5, sc=SIGMA_COLOR, sp=SIGMA_PLANE, reserved=(0, 0, 0, 0), null=False):
        dp = rt.DenoiseParams(levels, npow, sc, sp, (C.c_uint32 * 4)(*reserved))
        return rt.lib.rtx_denoise(c._h, w, h, None if null else C.byref(dp), None)

    def read_rc():
        return (rt.lib.rtx_read_denoised(c._h, buf.ctypes.data_as(C.c_void_p), buf.nbytes), rt.lib.rtx_read_denoised_srgb8(c._h, buf8.ctypes.data_as(C.c_void_p), buf8.nbytes))
    try:
        assert rc() == STATE and read_rc() == (STATE, STATE), "before commit"
        c.set_materials(cornell.materials)
        for v, i, m in cornell.meshes:
            c.add_mesh(v, i, m)
        for mesh, o2w in cornell.instances:
            c.add_instance(mesh, o2w)
        c.commit()
        assert rc() == STATE, "before the camera"
        c.set_camera(*cornell.view_proj(ASPECT))
        assert rc() == STATE and read_rc() == (STATE, STATE), "before any accumulation"
        a = render(rt, c, 1)
        assert read_rc() == (STATE, STATE), "before a successful rtx_denoise"
        assert rc() == rt.RTX_OK and read_rc() == (0, 0)
        d0 = c.read_denoised()
        same_image(d0, ref.emulate(a, ref.cornell_guides(), 3)[0], "the image the failing calls must leave")
        nan, inf = float("nan"), float("inf")
        bad = [dict(w=W + 1), dict(h=H - 1), dict(w=0, h=0), dict(levels=9), dict(npow=8), dict(sc=-1.0), dict(sc=nan), dict(sc=inf), dict(sp=-0.5), dict(sp=nan), dict(sp=inf),
               dict(sc=1e-45), dict(sp=1e-45), dict(reserved=(0, 0, 1, 0)), dict(reserved=(7, 0, 0, 0))]
        for kw in bad:
            assert rc(**kw) == INVALID, kw
            assert rt.lib.rtx_last_error(c._h)
        same_image(c.read_denoised(), d0, "after the invalid calls"); same_image(c.read_accum(), a, "u1 after the invalid calls")
        c.set_instance_visible(0, False)                            # a scene edit that is not committed yet
        assert rc() == STATE and rc(null=True) == STATE
        with pytest.raises(rt.RtxError):
            c.denoise(W, H)
        c.set_instance_visible(0, True); c.commit()
        same_image(c.read_denoised(), d0, "after the refused call"); same_image(c.read_accum(), a, "u1 after the refused call")
        assert rc(null=True) == rt.RTX_OK                           # NULL = every default
        assert rc() == rt.RTX_OK
        same_image(c.read_denoised(), d0, "the same call again")
        c.clear(37, 19)                                             # the accumulation buffer has another size now
        assert read_rc() == (STATE, STATE)
        assert rc() == INVALID
        c.clear(W, H)                                               # ... and the denoised image's again: it was never touched
        same_image(c.read_denoised(), d0, "after the clears")
    finally:
        c.close()


# ---- stream ----
def test_on_a_caller_bound_stream_behind_an_async_frame(rt, general):
    import torch
    p = rt.Params(**dict(BASE, spp=SPP, flags=1))
    a = render(rt, general, 1)
    general.denoise(W, H, 3, **KW)
    want = general.read_denoised()
    s = torch.cuda.Stream()
    general.set_stream(s.cuda_stream)
    general.set_option(rt.OPT_ASYNC, 1)
    try:
        general.clear(W, H)
        general.render(p)                                           # enqueued
        assert general.denoise(W, H, 3, result=False, **KW) is None  # enqueued behind it: no host join
        got = general.read_denoised()
        same_image(got, want, "async, caller-bound stream")
        general.render(p.copy(sample_base=BASE["sample_base"] + SPP))
        res = general.denoise(W, H, 3, **KW)                        # with a result the call joins the stream up to the denoise
        b = general.read_accum()
        assert (b[..., 3] == 2 * SPP)[a[..., 3] == SPP].all(), "the accumulation went on after the denoise"
        e, nf = ref.emulate(b, ref.cornell_guides(), 3)
        same_image(general.read_denoised(), e, "the second frame"); assert res.pixels_filtered == nf
    finally:
        general.set_option(rt.OPT_ASYNC, 0)
        general.set_stream(None)
        s.synchronize()


# ---- upper layers ----
def test_renderer_facade(rt, cornell):
    r = rt.Renderer(W, H, "denoise")
    try:
        r.set_scene(cornell)
        r.params.spp, r.params.flags, r.params.max_bounces, r.params.nee_samples = SPP, 1, 8, 1
        r.on_init(); r.on_update(); r.on_render()
        a = r.read_accum()
        d = r.read_denoised()
        sp = default_sigma_plane(cornell)
        same_image(d, ref.emulate(a, ref.cornell_guides(), 5, 0.5, sp, 5)[0], "Renderer.read_denoised")
        same_image(r.read_accum(), a, "u1 after Renderer.read_denoised")
    finally:
        r.close()


def test_cli_writes_the_denoised_image(rt, tmp_path):
    """rtx_render --denoise --out x.exr reads back equal to a Context doing the same"""
    exe = os.path.join(graft.PKG_DIR, "rtx_render")
    out = str(tmp_path / "x.exr")
    r = subprocess.run([exe, "--scene", "cornell", "--w", str(W), "--h", str(H), "--spp", "4", "--denoise", "--out", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
    assert "denoise: 5 levels" in r.stdout
    px = read_exr_rgb(out)
    sc = rt.Scene.cornell()
    c = rt.Context(0)
    try:
        c.upload(sc, W / H)
        c.clear(W, H)
        c.render(rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=rt.FLAG_LAMBERT_ONLY))
        res = c.denoise(W, H)
        d = c.read_denoised()
        assert f"{res.pixels_filtered} pixels filtered" in r.stdout
        assert np.array_equal(bits(px), bits(d[..., :3])), f"{int((bits(px) != bits(d[..., :3])).any(-1).sum())} pixels differ"
        assert not np.array_equal(bits(px), bits(ref.mean_of(c.read_accum())))
        # the native two-rank frame: rank 0 denoises the gathered image
        out2 = str(tmp_path / "x2.exr")
        r2 = subprocess.run([exe, "--scene", "cornell", "--w", str(W), "--h", str(H), "--spp", "4", "--gpus", "2", "--devices", "0,0", "--gather", "copy", "--denoise", "--out", out2],
                            capture_output=True, text=True, timeout=120)
        assert r2.returncode == 0, (r2.stdout[-1000:], r2.stderr[-1000:])
        assert open(out2, "rb").read() == open(out, "rb").read(), "--gpus 2 --denoise"
    finally:
        c.close()


def read_exr_rgb(path):
    """the float32 R, G, B planes of an uncompressed scanline OpenEXR file as host/ImageIO.cpp writes it -> (H, W, 3)"""
    b = open(path, "rb").read()
    assert b[:4] == bytes([0x76, 0x2F, 0x31, 0x01])
    pos, attrs = 8, {}
    while b[pos] != 0:
        e = b.index(b"\0", pos); name = b[pos:e].decode(); pos = e + 1
        e = b.index(b"\0", pos); typ = b[pos:e].decode(); pos = e + 1
        n = int.from_bytes(b[pos:pos + 4], "little"); pos += 4
        attrs[name] = (typ, b[pos:pos + n]); pos += n
    pos += 1
    assert attrs["compression"][1] == b"\0", "uncompressed"
    dw = np.frombuffer(attrs["dataWindow"][1], np.int32)
    w, h = int(dw[2] - dw[0] + 1), int(dw[3] - dw[1] + 1)
    chans, q, cb = [], 0, attrs["channels"][1]
    while cb[q] != 0:
        e = cb.index(b"\0", q); chans.append((cb[q:e].decode(), int.from_bytes(cb[e + 1:e + 5], "little"))); q = e + 1 + 16
    assert all(t == 2 for _, t in chans), "float channels"
    offs = np.frombuffer(b, np.uint64, h, pos)
    img = np.zeros((h, w, 3), np.float32)
    for y in range(h):
        o = int(offs[y])
        yy, n = int.from_bytes(b[o:o + 4], "little", signed=True), int.from_bytes(b[o + 4:o + 8], "little")
        row = np.frombuffer(b, np.float32, n // 4, o + 8).reshape(len(chans), w)
        for k, (name, _) in enumerate(chans):
            if name in "RGB":
                img[yy - int(dw[1]), :, "RGB".index(name)] = row[k]
    return img

"""rtx_denoise_variance on the GPU (include/rtx.h, DENOISING: VARIANCE-GUIDED) against the float32 twin of tests/denoise_var_ref.py: the adaptive state it reads, level 0's
(v, gv) and the denoised image bit for bit under every staging choice and flag word; threshold 0 as the fixed-spp route; rtx_denoise beside it unchanged; state and argument
errors; the upper layers.  The Cornell box (the tiny-scene guides) at 100 x 50, 37 x 19 (partial tiles on both axes) and 8 x 8 (smaller than one tile: every halo position
lies outside the image), and the two mapped variants of tests/denoise_maps_ref.py on the general path.  That the inputs are not vacuous is shown on the CPU
(tests/test_denoise_var_ref.py)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import denoise_maps_ref as mr
import denoise_var_ref as vr
import test_adaptive_ref as ar
import test_denoise_ref as ref
from test_adaptive_ref import ASPECT, BASE, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD
from test_denoise_ref import F, NOGEO
from test_normalmap import PT, context

pytestmark = pytest.mark.gpu
INVALID, STATE = -1, -4
SIZES = ((ar.W, ar.H), (37, 19), (8, 8))
LEVELS = (1, 3, 5)
LDS_STEPS = (0, 1, 2, 4)
VARIANTS = ("KD", "KD+CUT")
KW = dict(sigma_plane=ref.SIGMA_PLANE, normal_power_log2=ref.NORMAL_POWER_LOG2)        # the Cornell box; sigma_var stays at its default
MKW = dict(sigma_plane=mr.SIGMA_PLANE, normal_power_log2=mr.NORMAL_POWER_LOG2)         # the mapped room


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_image(a, b, what):
    d = bits(a) != bits(b)
    assert not d.any(), f"{what}: {int(d.any(-1).sum())} pixels differ (first at {tuple(np.argwhere(d.any(-1))[0])}; last channel differs in {int(d[..., -1].sum())})"


def ids(size):
    return f"{size[0]}x{size[1]}"


@pytest.fixture(scope="module")
def box(rt, cornell):
    c = rt.Context(0)
    c.upload(cornell, ASPECT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctxs(rt):
    cs = {name: context(rt, [], mr.variant(name)) for name in VARIANTS}
    yield cs
    for c in cs.values():
        c.close()


@functools.lru_cache(maxsize=None)
def tables(name):
    return mr.Tables(mr.variant(name))


def sample_box(rt, c, w=ar.W, h=ar.H, flags=1, ts=16, max_spp=MAX_SPP, threshold=THRESHOLD, **kw):
    """clear, then one rtx_render_adaptive of the Cornell box -> (u1, half)"""
    c.clear(w, h)
    c.render_adaptive(rt.Params(**dict(BASE, width=w, height=h, flags=flags, tile_size=ts, spp=77, **kw)), MIN_SPP, STEP_SPP, max_spp, threshold)
    return c.read_accum(), c.read_adaptive_half()


def sample_room(rt, c, w, h):
    c.clear(w, h)
    c.render_adaptive(rt.Params(**dict(PT, width=w, height=h, tile_size=16)), 4, 4, 12, 0.25)
    return c.read_accum(), c.read_adaptive_half()


def flags_kw(flags):
    return dict(albedo=bool(flags & mr.ALBEDO), mapped_normals=bool(flags & mr.MAPPED_NORMALS))


def check(rt, c, a, hb, g, mg, flags, kw, what, levels=LEVELS, lds_steps=LDS_STEPS):
    """denoise(variance=True) == the twin for every level count under every staging choice; counts exact"""
    h, w = a.shape[:2]
    d = None
    try:
        for lv in levels:
            e, nf = vr.emulate_var(a, hb, g, mg, lv, flags, **kw)
            for lds in lds_steps:
                c.set_option(rt.OPT_DENOISE_LDS_STEP, lds)
                res = c.denoise(w, h, lv, variance=True, **kw, **flags_kw(flags))
                d = c.read_denoised()
                same_image(d, e, f"{what}, flags {flags}, levels {lv}, LDS up to step {lds}")
                assert (res.levels, res.pixels_filtered, res.pixels_passed) == (lv, nf, w * h - nf), what
    finally:
        c.set_option(rt.OPT_DENOISE_LDS_STEP, 4)
    return d


def room_guides(rt, c, name, w, h):
    """the device's guide record and the twin's map guides from the device's own guide rays and closest hits (as tests/test_denoise_maps.py)"""
    rays = c.primary_rays(rt.Params(width=w, height=h, flags=0))
    hits = c.trace_closest(rays)
    g = c.denoise_guides(w, h)
    return g, mr.map_guides(tables(name), rays, hits, g)


# ---- 1: the state the filter reads ----
@pytest.mark.parametrize("ts", ar.TILES)
@pytest.mark.parametrize("flags", [1, 3])
def test_state_equals_the_emulation(rt, box, flags, ts):
    a, hb = sample_box(rt, box, flags=flags, ts=ts)
    e, _ = vr.emulate(flags, ts)
    assert np.array_equal(bits(e.accum), bits(ar.emulate(flags, ts)[0].accum))
    same_image(a, e.accum, f"u1, flags {flags}, tile {ts}")
    same_image(hb, e.half, f"half, flags {flags}, tile {ts}")
    assert hb[..., :3].any() and not np.array_equal(bits(hb), bits(a))


# ---- 2: level 0's variance and its prefilter ----
@pytest.mark.parametrize("albedo", [False, True])
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_level0_variance_equals_the_twin(rt, box, size, albedo):
    w, h = size
    a, hb = sample_box(rt, box, w, h)
    g, mg = box.denoise_guides(w, h), box.denoise_map_guides(w, h)
    got = box.denoise_variance_input(w, h, albedo=albedo)
    want = vr.level0(a, hb, g, mg, albedo)
    same_image(got, want, f"(v, gv), {w} x {h}, albedo {albedo}")
    filt = vr.filterable(a, g)
    assert filt.any() and not got[~filt].any() and got[filt].any()
    if albedo and (w, h) == SIZES[0]:
        assert not np.array_equal(bits(got), bits(box.denoise_variance_input(w, h))), "dividing by A changes v"


def test_level0_variance_of_a_textured_albedo(rt, ctxs):
    c = ctxs["KD"]
    w, h = mr.SIZES[0]
    a, hb = sample_room(rt, c, w, h)
    g, mg = room_guides(rt, c, "KD", w, h)
    same_image(c.denoise_variance_input(w, h, albedo=True), vr.level0(a, hb, g, mg, True), "(v, gv) under a map_Kd")


# ---- 3: the image ----
@pytest.mark.parametrize("size", SIZES, ids=ids)
def test_image_equals_the_twin_on_the_cornell_box(rt, box, size):
    w, h = size
    a, hb = sample_box(rt, box, w, h)
    d = check(rt, box, a, hb, box.denoise_guides(w, h), None, 0, KW, f"Cornell box {w} x {h}")
    same_image(box.read_accum(), a, "u1 after the denoise"); same_image(box.read_adaptive_half(), hb, "half after the denoise")
    assert (d[..., 3] == 1).all()


@pytest.mark.parametrize("size", mr.SIZES, ids=ids)
@pytest.mark.parametrize("name", VARIANTS)
def test_image_equals_the_twin_with_map_guides(rt, ctxs, name, size):
    c = ctxs[name]
    w, h = size
    a, hb = sample_room(rt, c, w, h)
    g, mg = room_guides(rt, c, name, w, h)
    plain = check(rt, c, a, hb, g, mg, 0, MKW, name, levels=(5,), lds_steps=(4,))
    for flags in (1, 2, 3):
        d = check(rt, c, a, hb, g, mg, flags, MKW, name)
        if size == mr.SIZES[0]:
            assert not np.array_equal(bits(d), bits(plain)), f"flags {flags} changes the image of this frame"
    same_image(c.read_accum(), a, "u1 after the denoise"); same_image(c.read_adaptive_half(), hb, "half after the denoise")


@pytest.mark.parametrize("name", VARIANTS)
def test_image_equals_the_twin_on_a_gpu_built_tree(rt, name):
    c = context(rt, [("OPT_GPU_BUILD", 1)], mr.variant(name))
    try:
        w, h = mr.SIZES[1]
        a, hb = sample_room(rt, c, w, h)
        g, mg = room_guides(rt, c, name, w, h)
        for flags in (1, 2, 3):
            check(rt, c, a, hb, g, mg, flags, MKW, f"{name}, GPU build", levels=(5,))
    finally:
        c.close()


# ---- 4: a fixed sample count, and rtx_denoise beside it ----
def test_threshold_zero_is_the_fixed_spp_route(rt, box):
    w, h = ar.W, ar.H
    box.clear(w, h)
    box.render(rt.Params(**dict(BASE, flags=1, spp=8)))
    fixed = box.read_accum()
    a, hb = sample_box(rt, box, max_spp=8, threshold=0.0)
    same_image(a, fixed, "rtx_render_adaptive with threshold 0 against rtx_render")
    g = box.denoise_guides(w, h)
    check(rt, box, a, hb, g, None, 0, KW, "threshold 0", levels=(5,), lds_steps=(4,))
    res = box.denoise(w, h, 5, sigma_color=ref.SIGMA_COLOR, **KW)
    e, nf = ref.emulate(a, g, 5)
    same_image(box.read_denoised(), e, "rtx_denoise after rtx_denoise_variance")
    assert res.pixels_filtered == nf


@pytest.mark.parametrize("lds", [4, 0])
def test_the_two_filters_alternate_on_one_context(rt, box, lds):
    """Both filters go through one level launcher and share the context's guide, ping-pong and count buffers: rtx_denoise, rtx_denoise_variance, rtx_denoise again, flags 3,
    3 levels at 37 x 19 (partial tiles, clamped halos) — each image and count is its twin's, and the variance call leaves nothing behind that the third call picks up"""
    w, h = SIZES[1]
    a, hb = sample_box(rt, box, w, h)
    g, mg = box.denoise_guides(w, h), box.denoise_map_guides(w, h)
    want = {False: mr.emulate_maps(a, g, mg, 3, 3, sigma_color=ref.SIGMA_COLOR, **KW), True: vr.emulate_var(a, hb, g, mg, 3, 3, **KW)}
    got = []
    try:
        box.set_option(rt.OPT_DENOISE_LDS_STEP, lds)
        for variance in (False, True, False):
            kw = dict(variance=True) if variance else dict(sigma_color=ref.SIGMA_COLOR)
            res = box.denoise(w, h, 3, albedo=True, mapped_normals=True, **kw, **KW)
            got.append(box.read_denoised())
            e, nf = want[variance]
            same_image(got[-1], e, f"call {len(got)} (variance {variance}), LDS up to step {lds}")
            assert (res.levels, res.pixels_filtered, res.pixels_passed) == (3, nf, w * h - nf), f"call {len(got)}"
    finally:
        box.set_option(rt.OPT_DENOISE_LDS_STEP, 4)
    same_image(got[2], got[0], "rtx_denoise after rtx_denoise_variance against rtx_denoise before it")
    assert not np.array_equal(bits(got[1]), bits(got[0])), "the two filters differ on this frame"


# ---- 5: errors ----
def test_errors(rt, box):
    w, h = ar.W, ar.H
    c = box
    a, hb = sample_box(rt, c)
    c.denoise(w, h, 3, variance=True, **KW)
    d0 = c.read_denoised()
    out2 = np.zeros((h, w, 2), F)

    def call(levels=3, power=5, sigma_var=0.0, flags=0, reserved=(0, 0, 0)):
        vp = rt.DenoiseVarParams(levels, power, sigma_var, 0.02, flags, (C.c_uint32 * 3)(*reserved))
        rc = rt.lib.rtx_denoise_variance(c._h, w, h, C.byref(vp), None)
        assert rc == rt.RTX_OK or rt.lib.rtx_last_error(c._h)
        return rc
    assert call() == rt.RTX_OK
    same_image(c.read_denoised(), d0, "the same call again")
    for kw in (dict(flags=4), dict(flags=8), dict(flags=0x80000000), dict(reserved=(1, 0, 0)), dict(reserved=(0, 0, 1)), dict(levels=9), dict(power=8),
               dict(sigma_var=-1.0), dict(sigma_var=float("nan")), dict(sigma_var=float("inf")), dict(sigma_var=1e-45)):
        assert call(**kw) == INVALID, kw
    assert rt.lib.rtx_denoise_variance(c._h, w + 1, h, None, None) == INVALID
    assert rt.lib.rtx_debug_denoise_variance(c._h, w, h, 4, out2.ctypes.data_as(C.c_void_p)) == INVALID and rt.lib.rtx_debug_denoise_variance(c._h, w, h, 0, None) == INVALID
    assert rt.lib.rtx_read_adaptive_half(c._h, out2.ctypes.data_as(C.c_void_p), out2.nbytes) == INVALID, "buffer too small"
    same_image(c.read_accum(), a, "u1 after the invalid calls"); same_image(c.read_adaptive_half(), hb, "half after the invalid calls")
    same_image(c.read_denoised(), d0, "the denoised image after the invalid calls")

    def refused(what):
        half = np.zeros((h, w, 4), F)
        assert call() == STATE, what
        assert rt.lib.rtx_read_adaptive_half(c._h, half.ctypes.data_as(C.c_void_p), half.nbytes) == STATE, what
        assert rt.lib.rtx_debug_denoise_variance(c._h, w, h, 0, out2.ctypes.data_as(C.c_void_p)) == STATE, what
        same_image(c.read_denoised(), d0, f"the denoised image, {what}")
    c.render(rt.Params(**dict(BASE, flags=1, spp=2)))                  # u1 now holds samples `half` does not know
    mixed = c.read_accum()
    refused("after rtx_render")
    same_image(c.read_accum(), mixed, "u1 after the refused calls")
    c.clear(w, h)
    refused("after rtx_clear_accum")
    c.render_adaptive(rt.Params(**dict(BASE, flags=1, tile_size=16, shard_rank=0, shard_count=2)), MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD)
    sharded = c.read_accum()
    refused("after a sharded rtx_render_adaptive")
    same_image(c.read_accum(), sharded, "u1 after the refused calls")
    a2, hb2 = sample_box(rt, c)                                        # a clear and an unsharded call make it whole again
    same_image(a2, a, "u1 after the clear"); same_image(hb2, hb, "half after the clear")
    assert call() == rt.RTX_OK
    same_image(c.read_denoised(), d0, "the denoised image after the clear")
    with pytest.raises(ValueError):
        c.denoise(w, h, variance=True, sigma_color=0.5)


# ---- 6: the upper layers ----
def test_renderer_facade(rt, cornell):
    """Renderer::DenoiseVariance through its C wrapper: the twin's image of the renderer's own state; refused once OnRender has added rtx_render's samples"""
    w, h = ar.W, ar.H
    r = rt.Renderer(w, h, "denoise variance")
    view = rt.Context.__new__(rt.Context)                          # a borrowed view of the renderer's context: never closed from here
    view._h, view.width, view.height = None, w, h
    try:
        r.set_scene(cornell)
        r.params.spp, r.params.flags, r.params.max_bounces, r.params.nee_samples = 2, 1, 8, 1
        r.on_init(); r.on_update()
        view._h = rt.lib.rtxh_renderer_context(r._h)
        a, hb = sample_box(rt, view)
        res = r.denoise_variance(levels=3, albedo=True, **KW)
        g, mg = view.denoise_guides(w, h), view.denoise_map_guides(w, h)
        e, nf = vr.emulate_var(a, hb, g, mg, 3, 1, **KW)
        same_image(view.read_denoised(), e, "Renderer::DenoiseVariance")
        assert (res.levels, res.pixels_filtered) == (3, nf)
        r.on_render()
        with pytest.raises(rt.RtxError):
            r.denoise_variance()
        assert rt.lib.rtxh_renderer_denoise_variance(r._h, None, None) == INVALID
    finally:
        view._h = None
        r.close()


def test_cli(rt, tmp_path):
    """rtx_render --adaptive T --denoise-variance writes an image that differs from the plain --denoise one; without --adaptive, or on several GPUs, it is a usage error"""
    from test_denoise import read_exr_rgb
    exe = os.path.join(graft.PKG_DIR, "rtx_render")
    base = [exe, "--scene", "cornell", "--w", "100", "--h", "50", "--spp", "8", "--adaptive", "0.25", "--min-spp", "4", "--step-spp", "4"]

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out", out] + list(extra), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out), r.stdout
    plain, _ = cli("p.exr", "--denoise")
    var, log = cli("v.exr", "--denoise-variance", "--sigma-var", "4", "--denoise-albedo")
    assert "variance-guided" in log and np.isfinite(var).all() and var.sum() > 0 and not np.array_equal(bits(var), bits(plain))
    for args in (["--scene", "cornell", "--denoise-variance"], ["--scene", "cornell", "--denoise-variance", "--gpus", "2"], ["--scene", "cornell", "--adaptive", "0.25", "--denoise-variance", "--gpus", "2"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--adaptive" in r.stderr, (args, r.returncode, r.stderr[-300:])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise-variance" in r.stdout and "--sigma-var" in r.stdout

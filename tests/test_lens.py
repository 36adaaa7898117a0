"""The thin-lens camera on the GPU (include/rtx.h, THIN LENS): rays and seeds against the numpy twin tests/lens_ref.py bit for bit, whole frames against the oracle's tracer
on the twin's rays bit for bit on every schedule (tiny fused, general, jitter, compact state, sample interleave, batches, shards, adaptive passes), radius 0 == no lens,
who ignores the lens, state and errors, autofocus, the command line.  Images are at most 64 x 48."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import lens_ref
from test_lens_ref import QuadScene, facing_quad

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H, SPP = 64, 48, 8
FOVY = math.radians(60.0)
R, F = 0.6, 6.0                       # circle of confusion of the emitter at depth 2: R |2 - F| / 2 * (H / 2) / (F tan(fovy / 2)) = 8.3 px
KE = (4.0, 2.0, 1.0)
EXE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
ERR_INVALID, ERR_STATE = -1, -4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_image(a, b, what):
    d = bits(a) != bits(b)
    assert not d.any(), f"{what}: {int(d.any(-1).sum())} pixels differ (w differs in {int(d[..., 3].sum())})"


def counts(ctx):
    st = ctx.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def launches(ctx):
    return tuple(ctx.stats().kernel_launches)


# ---- the scene of the whole-frame check: a front-facing emissive quad at depth 2, two black quads at depth 1 that partly occlude it, a black back wall ----
FRAME_QUADS = [facing_quad(0.0, 0.0, -2.0, 0.12, 0.12, 0),
               facing_quad(0.175, 0.0, -1.0, 0.125, 0.3, 1), facing_quad(-0.16, 0.15, -1.0, 0.14, 0.15, 1),
               facing_quad(0.0, 0.0, -8.0, 20.0, 20.0, 1)]


def frame_scene(rt):
    view = rt.lookat((0.0, 0.0, 0.0), (0.0, 0.0, -1.0), (0.0, 1.0, 0.0))
    proj = rt.perspective_fov_rh(FOVY, W / H, 0.1, 1000.0)
    return QuadScene([((0, 0, 0), KE), ((0, 0, 0), (0, 0, 0))], FRAME_QUADS, view, proj)


def frame_params(rt, flags, **kw):
    return rt.Params(**dict(dict(width=W, height=H, spp=SPP, sample_base=1, max_bounces=2, nee_samples=1, frame_seed=7, flags=flags, tile_size=16), **kw))


def running_sum(c, n):
    """the float32 sequential sum of n copies of c, for every n in 0 .. len - 1 -> (n + 1, 3)"""
    out = np.zeros((n + 1, 3), F32)
    for k in range(1, n + 1):
        out[k] = out[k - 1] + np.asarray(c, F32)
    return out


@pytest.fixture(scope="module")
def frame_ref(rt, orc):
    """per flag set (Lambert, Lambert + jitter): the expected accumulation of the lens frame, computed on the CPU — and, first, the premise it rests on"""
    sc = frame_scene(rt)
    o = orc.Oracle().load(sc, W / H)
    # PREMISE (pinhole render, the test's max_bounces and nee_samples): every pixel is 0 or the float32 running sum of SPP copies of ONE value c
    pin, _ = o.render(frame_params(rt, 1))
    sums = running_sum(KE, SPP)
    lit = pin[..., :3].any(-1)
    assert lit.any() and np.array_equal(bits(pin[lit][:, :3]), bits(np.broadcast_to(sums[SPP], (int(lit.sum()), 3)))) and (pin[..., 3] == SPP).all()
    out = {}
    for flags in (1, 1 | lens_ref.JITTER):
        p = frame_params(rt, flags)
        n = np.zeros(W * H, np.int64)
        for s in range(1, SPP + 1):
            rays, _, _ = lens_ref.lens_rays(orc, o, p, s, sc.view, R, F)
            n += o.trace_closest(rays, 0)[:, 3].view(np.uint32) < 2                 # triangles 0 and 1 are the emitter
        acc = np.zeros((H, W, 4), F32)
        acc[..., :3] = sums[n].reshape(H, W, 3)
        acc[..., 3] = SPP
        out[flags] = (acc, n.reshape(H, W))
    # a stale culling mask or a shared primary record would show: some pixel the pinhole never lights is lit through the lens in an 8 x 8 block that holds no pinhole-lit pixel
    n0 = out[1][1]
    blocks_lit = {(y // 8, x // 8) for y, x in zip(*np.nonzero(lit))}
    fresh = [(y, x) for y, x in zip(*np.nonzero((n0 > 0) & ~lit)) if (y // 8, x // 8) not in blocks_lit]
    assert fresh, "the lens lights no pixel outside the pinhole-lit blocks: choose a larger radius"
    print("pinhole-lit pixels", int(lit.sum()), "lens-lit", int((n0 > 0).sum()), "of them in blocks the pinhole leaves dark", len(fresh))      # 19, 69, 14
    return out


@pytest.fixture(scope="module")
def tiny(rt):
    c = rt.Context(0)
    c.upload(frame_scene(rt), W / H)
    yield c
    c.close()


@pytest.fixture(scope="module")
def general(rt):
    c = rt.Context(0)
    c.set_option(rt.OPT_SMALL_SCENE, 0)
    c.upload(frame_scene(rt), W / H)
    yield c
    c.close()


def lens_frame(rt, ctx, p, lens=(R, F)):
    ctx.set_lens(*lens) if lens else ctx.set_lens(None)
    ctx.clear(p.width, p.height)
    ctx.render(p)
    return ctx.read_accum()


# ---- 1. rays and seeds to the bit ----
@pytest.mark.parametrize("flags", [0, lens_ref.JITTER])
def test_rays_and_seeds_equal_the_twin(rt, orc, flags):
    w, h = 37, 23
    view = rt.lookat((1.5, 0.8, 2.5), (0.1, 0.2, -0.3), (0.0, 1.0, 0.0))
    proj = rt.perspective_fov_rh(math.radians(55.0), w / h, 0.1, 1000.0)
    o = orc.Oracle(); o.set_camera(view, proj)
    c = rt.Context(0)
    c.set_camera(view, proj)
    p = rt.Params(width=w, height=h, frame_seed=11, flags=flags)
    try:
        for s in (1, 2, 7):
            c.set_lens(0.3, 2.75)
            rays, seeds, q = lens_ref.lens_rays(orc, o, p, s, view, 0.3, 2.75)
            assert not q["kept"].any()
            assert np.array_equal(bits(c.primary_rays(p, s)), bits(rays)), f"rays, sample {s}"
            assert np.array_equal(c.primary_seeds(p, s), seeds), f"seeds, sample {s}"
            c.set_lens(0.0, 2.75)
            assert np.array_equal(bits(c.primary_rays(p, s)), bits(o.primary_rays(p, s))), f"radius 0: rays, sample {s}"
            assert np.array_equal(c.primary_seeds(p, s), lens_ref.seeds_without_lens(orc, w, h, s, 11, flags)), f"radius 0: seeds, sample {s}"
    finally:
        c.close()


# ---- 2. radius 0 is the pinhole ----
@pytest.mark.parametrize("kind", ["cornell_tiny", "cornell_general", "atrium"])
def test_radius_zero_is_the_pinhole(rt, cornell, kind):
    sc = rt.Scene.sponza_class(6000, 260) if kind == "atrium" else cornell
    p = rt.Params(width=W, height=H, spp=4, max_bounces=4, nee_samples=1, flags=1 if kind != "atrium" else 0, frame_seed=3)
    got = []
    for with_lens in (False, True):
        c = rt.Context(0)
        if kind == "cornell_general":
            c.set_option(rt.OPT_SMALL_SCENE, 0)
        c.upload(sc, W / H)
        if with_lens:
            c.set_lens(0.0, 3.0)
        c.clear(W, H); c.render(p)
        got.append((c.read_accum(), counts(c), launches(c)))
        c.close()
    (a, ca, la), (b, cb, lb) = got
    same_image(a, b, kind)
    assert ca == cb and la == lb, (ca, cb, la, lb)
    assert a[..., :3].max() > 0
    if kind == "cornell_tiny":
        assert la[rt.K_RAYGEN] == 2 and la[rt.K_TRACE] == 0, "the shared primary hit is still in use: its pre-pass and the queue-only raygen"


# ---- 3. a whole frame to the bit, through the oracle's tracer ----
def test_frame_on_the_tiny_fused_path(rt, tiny, frame_ref):
    img = lens_frame(rt, tiny, frame_params(rt, 1))
    st = tiny.stats()
    assert st.kernel_launches[rt.K_BOUNCE] > 0 and st.kernel_launches[rt.K_TRACE] == 0, "not the fused tiny-scene path"
    assert st.rays_primary == W * H * SPP
    same_image(img, frame_ref[1][0], "tiny fused")
    same_image(lens_frame(rt, tiny, frame_params(rt, 3)), frame_ref[3][0], "tiny fused, jitter")
    tiny.set_option(rt.OPT_SHARED_PRIMARY, 0)
    try:
        same_image(lens_frame(rt, tiny, frame_params(rt, 1)), frame_ref[1][0], "tiny fused, shared primary off")
    finally:
        tiny.set_option(rt.OPT_SHARED_PRIMARY, 1)


@pytest.mark.parametrize("flags", [1, 3])
@pytest.mark.parametrize("interleave,compact", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_frame_on_the_general_path(rt, general, frame_ref, interleave, compact, flags):
    general.set_option(rt.OPT_SAMPLE_INTERLEAVE, interleave)
    general.set_option(rt.OPT_COMPACT_STATE, compact)
    try:
        img = lens_frame(rt, general, frame_params(rt, flags))
        st = general.stats()
        assert st.kernel_launches[rt.K_TRACE] > 0 and st.kernel_launches[rt.K_BOUNCE] == 0, "not the general path"
        assert st.rays_primary == W * H * SPP
        same_image(img, frame_ref[flags][0], f"general, interleave {interleave}, compact {compact}, flags {flags}")
    finally:
        general.set_option(rt.OPT_SAMPLE_INTERLEAVE, 1)
        general.set_option(rt.OPT_COMPACT_STATE, 1)


def test_frame_with_the_fused_bvh_kernel(rt, general, frame_ref):
    general.set_option(rt.OPT_FUSED_BVH, 1)
    try:
        same_image(lens_frame(rt, general, frame_params(rt, 1)), frame_ref[1][0], "general, RTX_OPT_FUSED_BVH")
    finally:
        general.set_option(rt.OPT_FUSED_BVH, 0)


@pytest.mark.parametrize("path", ["tiny", "general"])
def test_frame_in_many_batches(rt, tiny, general, frame_ref, path):
    ctx = tiny if path == "tiny" else general
    ctx.set_option(rt.OPT_PATHS_PER_BATCH, 4096)               # 12 tiles of 16 x 16 = 3072 slots: one sample per batch, eight batches
    try:
        same_image(lens_frame(rt, ctx, frame_params(rt, 1)), frame_ref[1][0], f"{path}: eight batches")
    finally:
        ctx.set_option(rt.OPT_PATHS_PER_BATCH, 128 << 20)


@pytest.mark.parametrize("path", ["tiny", "general"])
def test_frame_from_three_shards(rt, tiny, general, frame_ref, path):
    ctx = tiny if path == "tiny" else general
    ctx.set_lens(R, F)
    ctx.clear(W, H)
    prim = 0
    for r in range(3):
        ctx.render(frame_params(rt, 1, shard_rank=r, shard_count=3))
        prim += ctx.stats().rays_primary
    assert prim == W * H * SPP
    same_image(ctx.read_accum(), frame_ref[1][0], f"{path}: shards 0..2 of 3")


@pytest.mark.parametrize("path", ["tiny", "general"])
def test_frame_by_adaptive_passes(rt, tiny, general, frame_ref, path):
    ctx = tiny if path == "tiny" else general
    ctx.set_lens(R, F)
    ctx.clear(W, H)
    res = ctx.render_adaptive(frame_params(rt, 1), 2, 2, SPP, 0.0)            # threshold 0 converges nothing: rtx_render's image of SPP samples
    assert res.passes == SPP // 2 and res.pixel_samples == W * H * SPP
    same_image(ctx.read_accum(), frame_ref[1][0], f"{path}: render_adaptive, threshold 0")


# ---- 4. downstream is untouched ----
def test_downstream_of_ray_generation_is_untouched(rt, cornell):
    """the Cornell box with its real materials, lens on: the tiny path and the general path agree to the bit (their parity contract), one shard and three agree"""
    base = dict(width=W, height=H, spp=8, max_bounces=4, nee_samples=1, flags=0, frame_seed=5, tile_size=16)
    imgs = {}
    for small in (1, 0):
        c = rt.Context(0)
        c.set_option(rt.OPT_SMALL_SCENE, small)
        c.upload(cornell, W / H)
        c.set_lens(0.05, 1.6)
        c.clear(W, H); c.render(rt.Params(**base))
        st = c.stats()
        assert st.rays_primary == W * H * 8 and (st.kernel_launches[rt.K_BOUNCE] > 0) == bool(small)
        imgs[small] = c.read_accum()
        c.clear(W, H)
        for r in range(3):
            c.render(rt.Params(shard_rank=r, shard_count=3, **base))
        same_image(c.read_accum(), imgs[small], f"small {small}: 3 shards vs 1")
        if small:
            c.set_lens(None); c.clear(W, H); c.render(rt.Params(**base))
            assert not np.array_equal(bits(c.read_accum()), bits(imgs[1])), "the lens changes nothing"
        c.close()
    same_image(imgs[1], imgs[0], "tiny path vs general path")


# ---- 5. who ignores the lens ----
def test_who_ignores_the_lens(rt, cornell):
    c = rt.Context(0)
    c.upload(cornell, W / H)
    p = rt.Params(width=W, height=H, spp=1, max_bounces=2, nee_samples=2, flags=1, frame_seed=2)
    got = []
    for lens in (None, (0.05, 1.6)):
        c.set_lens(*lens) if lens else c.set_lens(None)
        c.clear(W, H); c.render_v6_pass1(p)
        got.append((c.read_accum(), c.denoise_guides(W, H), c.read_layer(10, W, H)))
    c.close()
    assert got[0][0][..., :3].max() > 0
    same_image(got[0][0], got[1][0], "rtx_render_v6_pass1")
    assert np.array_equal(bits(got[0][1]), bits(got[1][1])), "denoise guides"
    assert np.array_equal(got[0][2], got[1][2]) and got[0][2][..., :3].any(), "layer 10"


# ---- 6. state and errors ----
def test_invalid_lenses_leave_the_previous_one(rt, tiny, frame_ref):
    p = frame_params(rt, 1)
    same_image(lens_frame(rt, tiny, p), frame_ref[1][0], "before")
    nan, inf = float("nan"), float("inf")
    bad = [rt.Lens(-0.1, 3.0), rt.Lens(nan, 3.0), rt.Lens(inf, 3.0), rt.Lens(0.5, 0.0), rt.Lens(0.5, -2.0), rt.Lens(0.5, nan), rt.Lens(0.5, inf), rt.Lens(0.0, nan),
           rt.Lens(0.5, 3.0, (C.c_uint32 * 2)(1, 0)), rt.Lens(0.5, 3.0, (C.c_uint32 * 2)(0, 7))]
    for lens in bad:
        assert rt.lib.rtx_set_lens(tiny._h, C.byref(lens)) == ERR_INVALID, (lens.aperture_radius, lens.focus_distance, list(lens.reserved))
        tiny.clear(W, H); tiny.render(p)
        same_image(tiny.read_accum(), frame_ref[1][0], "after an invalid lens")
    with pytest.raises(rt.RtxError):
        tiny.set_lens(-1.0, 3.0)


def test_lens_is_camera_state(rt):
    """on a resident general scene set_lens changes neither the refit count nor the tree and needs no commit; it survives set_camera; set_lens(None) is the pinhole again"""
    sc = rt.Scene.sponza_class(6000, 260)
    p = rt.Params(width=W, height=H, spp=2, max_bounces=3, nee_samples=1, flags=0, frame_seed=9)
    c = rt.Context(0)
    c.upload(sc, W / H)
    c.clear(W, H); c.render(p)
    pinhole, refits, tree = c.read_accum(), c.stats().bvh_refits, c.tree_hash()
    c.set_lens(0.2, 4.0)
    assert c.stats().bvh_refits == refits and c.tree_hash() == tree
    c.clear(W, H); c.render(p)                                   # no commit in between
    with_lens = c.read_accum()
    assert c.stats().bvh_refits == refits and c.tree_hash() == tree
    assert not np.array_equal(bits(with_lens), bits(pinhole))
    c.set_camera(*sc.view_proj(W / H))
    c.clear(W, H); c.render(p)
    same_image(c.read_accum(), with_lens, "the lens survives set_camera")
    c.set_lens(None)
    c.clear(W, H); c.render(p)
    same_image(c.read_accum(), pinhole, "set_lens(None)")
    assert counts(c)[0] == W * H * 2
    c.close()


# ---- 7. autofocus ----
def test_autofocus(rt, orc, cornell):
    c = rt.Context(0)
    assert rt.lib.rtx_focus_distance_at(c._h, W, H, 1, 1, C.byref(C.c_float())) == ERR_STATE
    c.upload(cornell, W / H)
    o = orc.Oracle().load(cornell, W / H)
    view, _ = cornell.view_proj(W / H)
    Vi = orc.mat4_inverse(view)
    rays = o.primary_rays(rt.Params(width=W, height=H, flags=0), 1)
    hits = o.trace_closest(rays, 0)
    miss = hits[:, 3].view(np.uint32) == 0xFFFFFFFF
    d = rays[:, 4:7]
    cz = np.abs((d[:, 0] * Vi[8] + d[:, 1] * Vi[9]) + d[:, 2] * Vi[10])
    want = np.where(miss, F32(0.0), hits[:, 0] * cz).astype(F32)
    assert miss.any() and not miss.all()
    hit_ids = np.flatnonzero(~miss)
    pixels = [int(np.flatnonzero(miss)[0])] + [int(hit_ids[k]) for k in (0, len(hit_ids) // 3, len(hit_ids) // 2, len(hit_ids) - 1)]
    c.set_lens(0.3, 2.0)                                          # the pinhole ray, lens or not
    for i in pixels:
        got = c.focus_distance_at(W, H, i % W, i // W)
        assert bits(got) == bits(want[i]), (i % W, i // W, float(got), float(want[i]))
    assert c.focus_distance_at(W, H, pixels[0] % W, pixels[0] // W) == 0.0
    for x, y in ((W, 0), (0, H), (1 << 30, 1)):
        assert rt.lib.rtx_focus_distance_at(c._h, W, H, x, y, C.byref(C.c_float())) == ERR_INVALID
    c.close()


# ---- 8. command line ----
def obj_of_the_frame_scene():
    """the frame scene as an OBJ, moved in front of the camera an OBJ scene gets (eye (-1.5, 1.5, 3.5) looking at (0, 1, 0): host/Scenes.cpp) as it stands in front of frame_scene's"""
    eye, ctr = np.array([-1.5, 1.5, 3.5]), np.array([0.0, 1.0, 0.0])
    fw = (ctr - eye) / np.linalg.norm(ctr - eye)
    rg = np.cross(fw, [0.0, 1.0, 0.0]); rg /= np.linalg.norm(rg)
    up = np.cross(rg, fw)
    v, f = [], []
    mats = ["lamp", "black", "black", "wall"]
    for k, (a, b, c, d, _) in enumerate(FRAME_QUADS):
        for q in (a, b, c, d):
            v.append("v %.9g %.9g %.9g" % tuple(eye + q[0] * rg + q[1] * up - q[2] * fw))
        f.append(f"usemtl {mats[k]}\nf {4 * k + 1} {4 * k + 2} {4 * k + 3} {4 * k + 4}")
    return "mtllib lens.mtl\n" + "\n".join(v) + "\n" + "\n".join(f) + "\n"


LENS_MTL = "newmtl lamp\nKd 0 0 0\nKe 4 2 1\nnewmtl black\nKd 0.05 0.05 0.05\nnewmtl wall\nKd 0.5 0.4 0.3\n"


def test_command_line(rt, tmp_path):
    """rtx_render --aperture R --focus D on the frame scene as an OBJ == the Python frame with set_lens(R, D), on one context and on the native two-rank frame;
    --focus-pixel prints the distance of focus_distance_at and focuses there"""
    from test_denoise import read_exr_rgb
    (tmp_path / "lens.obj").write_text(obj_of_the_frame_scene())
    (tmp_path / "lens.mtl").write_text(LENS_MTL)
    base = [EXE, "--obj", str(tmp_path / "lens.obj"), "--mtl", str(tmp_path), "--w", str(W), "--h", str(H), "--spp", "4", "--bounces", "3"]

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out", out] + list(extra), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out), r.stdout

    sc = rt.Scene.from_obj([str(tmp_path / "lens.obj")], str(tmp_path) + "/")
    p = rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=3, nee_samples=1, rr_start=3, frame_seed=1, flags=0)
    c = rt.Context(0)
    c.upload(sc, W / H)

    def python(lens):
        c.set_lens(*lens) if lens else c.set_lens(None)
        c.clear(W, H); c.render(p)
        a = c.read_accum()
        return a[..., :3] / np.maximum(a[..., 3:], F32(1.0))

    pinhole, focused = python(None), python((0.25, 2.5))
    assert focused.sum() > 0 and not np.array_equal(bits(pinhole), bits(focused))
    assert np.array_equal(bits(cli("a.exr", "--aperture", "0.25", "--focus", "2.5")[0]), bits(focused))
    assert np.array_equal(bits(cli("b.exr", "--aperture", "0.25", "--focus", "2.5", "--gpus", "2", "--devices", "0,0", "--gather", "copy")[0]), bits(focused))
    assert np.array_equal(bits(cli("c.exr")[0]), bits(pinhole))
    x, y = W // 2, H // 2
    dist = c.focus_distance_at(W, H, x, y)
    assert dist > 0
    img, text = cli("d.exr", "--aperture", "0.25", "--focus-pixel", f"{x},{y}")
    m = re.search(r"autofocus: pixel (\d+),(\d+) is at view depth (\S+)", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (x, y) and F32(float(m.group(3))) == dist, text
    assert np.array_equal(bits(img), bits(python((0.25, float(dist)))))
    img, _ = cli("e.exr", "--aperture", "0.25", "--focus-pixel", f"{x},{y}", "--focus", "2.5")            # an explicit --focus wins
    assert np.array_equal(bits(img), bits(focused))
    c.close()
    r = subprocess.run([EXE, "--aperture", "0.25"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--focus" in r.stderr

"""Environment lighting on the device (include/rtx.h: rtx_set_environment).  The mapping, the tables, the sampler and the lookup are held to the numpy twin
(tests/env_ref.py) bit for bit; the transport — an extension the reference has nothing to say about — is pinned by its own properties: exact sums on primary misses, exact
zeros, exact power-of-two scaling, a white furnace, a sun behind a blocker, and invariance under everything that must not change an image."""
import math
import os
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import env_ref as er
from test_deform import ArrayScene, bits
from test_denoise import read_exr_rgb
from test_env_ref import pfm_bytes, random_map, rotation, special_directions, unit
from test_texture import MAPS, SIZES, SRGB, TexScene, make_general, noise_texture

pytestmark = pytest.mark.gpu

W, H = 96, 64
F = np.float32
MISS = np.uint32(0xFFFFFFFF)
PT = dict(width=W, height=H, spp=4, max_bounces=4, nee_samples=1, rr_start=2)


def plain_material(rt, kd):
    """a non-emissive material as the scene generators make them: Kd, dissolve 1 | Ks | Ni | Ke = 0 | roughness 0.5 | the multiscatter table of that roughness"""
    m = np.zeros(32, np.float32)
    m[0:4] = (kd, kd, kd, 1.0); m[4:7] = 0.04; m[7] = 1.0; m[12] = 0.5
    m[16:32] = rt.generate_ess_lut(0.5)
    return m


def camera(rt, eye, center, up=(0.0, 1.0, 0.0), fov_deg=45.0):
    return lambda aspect: (rt.lookat(eye, center, up), rt.perspective_fov_rh(math.radians(fov_deg), aspect, 0.1, 100.0))


def grid_face(c, u, v, k, base_vertex):
    """a k x k grid of quads over the square c + s u + t v, s, t in [-1, 1]; the triangles wind so that the flat normal is cross(u, v)"""
    c, u, v = np.asarray(c, np.float64), np.asarray(u, np.float64), np.asarray(v, np.float64)
    s = np.linspace(-1.0, 1.0, k + 1)
    pos = np.array([c + a * u + b * v for b in s for a in s])
    idx = []
    for b in range(k):
        for a in range(k):
            q = base_vertex + b * (k + 1) + a
            idx += [q, q + 1, q + k + 2, q, q + k + 2, q + k + 1]
    return pos, idx


def mesh_of(faces, matid):
    """faces: [(centre, u, v, k)] -> (verts (n, 7) with zero vertex normals = flat shading, indices, one material id per index entry); a single mesh at materialIDs base 0"""
    pos, idx = [], []
    for c, u, v, k in faces:
        p, i = grid_face(c, u, v, k, sum(len(q) for q in pos))
        pos.append(p); idx += i
    vt = np.zeros((sum(len(q) for q in pos), 7), np.float32)
    vt[:, :3] = np.concatenate(pos)
    idx = np.array(idx, np.uint32)
    mids = np.asarray(matid, np.uint32)
    return vt, idx, (np.full(len(idx), mids, np.uint32) if mids.ndim == 0 else np.repeat(mids, 3))


IDENT = np.eye(4, dtype=np.float32).reshape(16)


def cube_scene(rt, floor=False):
    """a flat-shaded cube of 6 x 4 x 4 x 2 = 192 triangles, Kd = 0.5, seen from outside with background all around; floor: standing on a square of 8 more"""
    ax = np.eye(3)
    faces = [((0.0, -0.5, 0.0), (0.0, 0.0, 1.5), (1.5, 0.0, 0.0), 2)] if floor else []
    for n in range(3):
        for s in (1.0, -1.0):
            u, v = ax[(n + 1) % 3], ax[(n + 2) % 3]
            faces.append((s * ax[n] * 0.5, 0.5 * (u if s > 0 else v), 0.5 * (v if s > 0 else u), 4))      # cross(u, v) = the outward normal
    mesh = mesh_of(faces, 0)
    assert len(mesh[1]) == (200 if floor else 192) * 3
    return ArrayScene(np.array([plain_material(rt, 0.5)]), [mesh], [(0, IDENT)], camera(rt, (1.9, 1.4, 2.3), (0.0, 0.0, 0.0)), -2.0, 2.0)


# the sun-and-blocker scene: a floor at y = 0 and a black wall standing on it across the sun's azimuth; chosen in numpy (see test_sun_and_blocker) so that the penumbra stays small
WALL_HALF_WIDTH, WALL_HEIGHT, FLOOR_HALF = 1.5, 4.0, 2.0
WALL_N = np.array([-1.0, 0.0, 1.0]) / math.sqrt(2.0)
WALL_C = np.array([0.0, (WALL_HEIGHT - 0.05) / 2.0, 0.0])
WALL_EX = np.array([1.0, 0.0, 1.0]) / math.sqrt(2.0) * WALL_HALF_WIDTH
WALL_EY = np.array([0.0, (WALL_HEIGHT + 0.05) / 2.0, 0.0])


def sun_scene(rt):
    floor = ((0.0, 0.0, 0.0), (0.0, 0.0, FLOOR_HALF), (FLOOR_HALF, 0.0, 0.0), 1)          # cross(z, x) = +y
    wall = (WALL_C, WALL_EX, WALL_EY, 1)
    mesh = mesh_of([floor, wall], np.array([0, 0, 1, 1]))
    return ArrayScene(np.array([plain_material(rt, 0.5), plain_material(rt, 0.0)]), [mesh], [(0, IDENT)], camera(rt, (0.0, 5.0, 0.01), (0.0, 0.0, 0.0), (0.0, 0.0, 1.0)), -2.0, 4.0)


def sun_map():
    m = np.zeros((8, 8, 3), np.float32)
    m[5, 2] = 1000.0
    return m


class EnvScene(TexScene):
    """TexScene + the environment attribute Context.upload binds"""
    def __init__(self, base, environment=None, uvs=None, textures=None, material_maps=None):
        super().__init__(base, uvs, textures, material_maps)
        self.environment = environment


class World:
    def __init__(self, rt, golden_dir):
        rng = np.random.default_rng(20261019)
        general, self._keep = make_general(rt, golden_dir)
        self.general = general
        # the atrium seen from outside: most of the image is background
        self.outside = ArrayScene(general.materials, general.meshes, general.instances, camera(rt, (3.2, 2.6, 4.1), (0.0, 0.4, 0.0)), general.lo, general.hi)
        self.cornell = rt.Scene.cornell()
        self.tiny = ArrayScene(self.cornell.materials, self.cornell.meshes, self.cornell.instances, self.cornell.view_proj, -1.0, 1.0)
        self.map8, self.map64 = random_map(rng, 8), random_map(rng, 64)
        self.rot8, self.rot64 = rotation(rng), rotation(rng)
        maps = [MAPS.get(m, -1) for m in range(len(general.materials))]
        self.textured = EnvScene(self.general, None, [rng.uniform(-2.0, 3.0, (len(m), 2)).astype(np.float32) for _, _, m in general.meshes],
                                 [(noise_texture(rng, h, w), s) for (h, w), s in zip(SIZES, SRGB)], maps)


@pytest.fixture(scope="module")
def world(rt, golden_dir):
    return World(rt, golden_dir)


def context(rt, scene, opts=(), env=None, aspect=W / H):
    c = rt.Context(0)
    for o, v in opts:
        c.set_option(getattr(rt, o), v)
    if env is not None:
        scene = EnvScene(scene, env, getattr(scene, "uvs", None), getattr(scene, "textures", None), getattr(scene, "material_maps", None))
    c.upload(scene, aspect)
    return c


def frame(rt, c, **kw):
    p = rt.Params(**dict(PT, **kw))
    c.clear(p.width, p.height)
    c.render(p)
    return c.read_accum()


def primary_hits(rt, c, **kw):
    """per pixel (row-major): the primary ray (o, d) and the hit record, from the device's own probes (no jitter: every sample shoots the same ray)"""
    rays = c.primary_rays(rt.Params(**dict(PT, **kw)))
    return rays, c.trace_closest(rays)


# ------------------------------------------------------------------------------------------------
# 1. tables, sampler and lookup against the twin, to the bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["map8", "map64"])
def test_probes_match_the_twin(rt, world, which):
    m, rot = getattr(world, which), getattr(world, "rot" + which[3:])
    assert (m.sum(-1) == 0).any()
    c = context(rt, world.tiny, env=dict(img=m, to_world=rot, scale=1.5))
    try:
        tab = er.Tables(m, 1.5, rot)
        tex, marg, cond = c.env_tables()
        assert np.array_equal(bits(tex), bits(tab.texels)) and np.array_equal(bits(marg), bits(tab.marginal)) and np.array_equal(bits(cond), bits(tab.conditional))
        rng = np.random.default_rng(11)
        seeds = rng.integers(0, 2 ** 32, (4096, 2), dtype=np.uint64).astype(np.uint32)
        out = c.env_sample(seeds)
        d, pdf, L, t, s0, s1 = tab.sample(seeds[:, 0], seeds[:, 1])
        assert np.array_equal(bits(out[:, 0:3]), bits(d)) and np.array_equal(bits(out[:, 3]), bits(pdf)) and np.array_equal(bits(out[:, 4:7]), bits(L))
        assert np.array_equal(bits(out[:, 7]), t.astype(np.uint32)) and (out[:, 10:12] == 0).all()
        assert (tab.w.ravel()[t] > 0).all() and (pdf > 0).all()
        a, b = seeds[:, 0], seeds[:, 1]
        for _ in range(4):                                        # the seed after a sample = four RandomFloat steps
            _, a, b = er.tea_next(a, b)
        assert np.array_equal(bits(out[:, 8]), a) and np.array_equal(bits(out[:, 9]), b) and np.array_equal(a, s0) and np.array_equal(b, s1)
        dirs = np.concatenate([unit(rng.normal(size=(4096, 3))), special_directions(), er.to_world(tab.R, special_directions())])
        ev = c.env_eval(dirs)
        L, pdf, t, r3 = tab.eval(dirs)
        assert np.array_equal(bits(ev[:, 0:3]), bits(L)) and np.array_equal(bits(ev[:, 3]), bits(pdf)) and np.array_equal(bits(ev[:, 4]), t.astype(np.uint32))
        assert np.array_equal(bits(ev[:, 5]), bits(r3)) and (ev[:, 6:8] == 0).all()
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 2. primary misses
# ------------------------------------------------------------------------------------------------
def test_primary_misses_hold_the_map(rt, world):
    env = dict(img=world.map64, to_world=world.rot64, scale=0.75)
    c = context(rt, world.outside, env=env)
    try:
        spp = 3
        rays, hits = primary_hits(rt, c)
        miss = hits[:, 3].view(np.uint32) == MISS
        assert 500 < miss.sum() < W * H - 500
        L = er.Tables(world.map64, 0.75, world.rot64).eval(rays[miss, 4:7])[0]
        want = np.zeros_like(L)
        for _ in range(spp):
            want = want + L
        img = frame(rt, c, max_bounces=1, spp=spp).reshape(-1, 4)
        assert np.array_equal(bits(img[miss, :3]), bits(want)) and (img[:, 3] == spp).all()
        lit = img[~miss, :3].copy()
        c.set_environment(hidden=True, **env); c.commit()
        img = frame(rt, c, max_bounces=1, spp=spp).reshape(-1, 4)
        assert (bits(img[miss, :3]) == 0).all() and (img[:, 3] == spp).all()
        assert np.array_equal(bits(img[~miss, :3]), bits(lit))      # hiding the backdrop changes no lighting
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 3. a black environment is no environment
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "tiny"])
def test_black_environment_equals_none(rt, world, name):
    opts = [("OPT_SMALL_SCENE", 0)] if name == "tiny" else []       # both runs on the general path: an environment moves a tiny scene there
    flags = rt.FLAG_LAMBERT_ONLY if name == "tiny" else 0
    a = context(rt, getattr(world, name), opts)
    b = context(rt, getattr(world, name), opts, env=np.zeros((8, 8, 3), np.float32))
    try:
        ia, sa = frame(rt, a, flags=flags), a.stats()
        ib, sb = frame(rt, b, flags=flags), b.stats()
        assert np.array_equal(bits(ia), bits(ib)) and ia[..., :3].max() > 0
        assert (sa.rays_primary, sa.rays_extension, sa.rays_shadow) == (sb.rays_primary, sb.rays_extension, sb.rays_shadow) and sa.rays_shadow > 0
        # ... and so is one whose scale is 0
        b.set_environment(world.map8, scale=0.0); b.commit()
        assert np.array_equal(bits(frame(rt, b, flags=flags)), bits(ia)) and b.stats().rays_shadow == sa.rays_shadow
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------------------------------
# 4. power-of-two scaling of a scene lit by the environment alone
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
def test_power_of_two_scaling(rt, world, flags):
    """a cube on a floor, no emissive triangle (the atrium will not do: its sky quad closes the opening whether it emits or not): lit by the environment alone"""
    c = context(rt, cube_scene(rt, floor=True), env=dict(img=world.map8, to_world=world.rot8))
    shot = lambda: frame(rt, c, flags=flags)
    try:
        assert c.stats().lights == 0
        one, st = shot(), c.stats()
        rays, hits = primary_hits(rt, c)
        hit = hits[:, 3].view(np.uint32) != MISS
        assert one.reshape(-1, 4)[hit, :3].max() > 0 and (one.reshape(-1, 4)[hit, :3].sum(-1) > 0).mean() > 0.5      # surfaces are lit: without the environment they are black
        assert st.rays_shadow > 0 and st.kernel_launches[rt.K_SHADOW] == PT["max_bounces"]      # one environment slot per bounce, no triangle-light slots
        four = one.copy(); four[..., :3] = one[..., :3] * F(4.0)
        c.set_environment(world.map8 * F(4.0), to_world=world.rot8); c.commit()
        assert np.array_equal(bits(shot()), bits(four))
        c.set_environment(world.map8, to_world=world.rot8, scale=4.0); c.commit()
        assert np.array_equal(bits(shot()), bits(four))
        c.set_environment(None); c.commit()
        dark = shot()
        assert (bits(dark[..., :3]) == 0).all() and c.stats().rays_shadow == 0
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 5. white furnace
# ------------------------------------------------------------------------------------------------
def test_white_furnace(rt):
    """a convex Lambert body (Kd = rho = 0.5) under a constant sky L = 1 leaves rho L: the environment NEE sample and the miss of the continuation ray, one sample each
    under the balance heuristic, add up to it.  A sample lies in [0, 2 rho], so its std is at most rho"""
    rho, spp = 0.5, 64
    c = context(rt, cube_scene(rt), env=np.ones((1, 1, 3), np.float32))
    try:
        kw = dict(flags=rt.FLAG_LAMBERT_ONLY, max_bounces=2, rr_start=2, spp=spp)
        rays, hits = primary_hits(rt, c, **kw)
        hit = hits[:, 3].view(np.uint32) != MISS
        assert 500 < hit.sum() < W * H - 1000
        img = frame(rt, c, **kw).reshape(-1, 4)
        assert (img[~hit, :3] == F(spp)).all() and (img[:, 3] == spp).all()
        mean = float((img[hit, :3].astype(np.float64) / spp).mean())
        tol = 6.0 * rho / math.sqrt(hit.sum() * spp)
        print(f"white furnace: mean {mean:.5f} over {hit.sum()} pixels, tolerance {tol:.5f}")
        assert (img[hit, :3] >= 0).all() and (img[hit, :3] <= 2.0 * rho * spp * (1 + 1e-5)).all()
        assert abs(mean - rho) <= tol
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 6. sun and blocker
# ------------------------------------------------------------------------------------------------
def wall_hits(p, d, margin):
    """(points, directions) -> the ray from the point along the direction meets the wall quad grown by `margin` on every side"""
    den = d @ WALL_N
    with np.errstate(divide="ignore", invalid="ignore"):
        t = ((WALL_C - p) @ WALL_N)[:, None] / den[None, :]
        P = p[:, None, :] + t[..., None] * d[None, :, :]
    lx, ly = ((P - WALL_C) @ WALL_EX) / (WALL_EX @ WALL_EX), ((P - WALL_C) @ WALL_EY) / (WALL_EY @ WALL_EY)
    return (np.abs(lx) <= 1.0 + margin / np.linalg.norm(WALL_EX)) & (np.abs(ly) <= 1.0 + margin / np.linalg.norm(WALL_EY)) & (t > 1e-9)


def test_sun_and_blocker(rt):
    """the 8 x 8 map whose only light is the texel (row 5, column 2) — a "sun" of 0.27 sr around (-0.64, 0.43, 0.64) that reaches down to the horizon — over a floor with a
    black wall across its azimuth.  In numpy: a floor pixel is in the UMBRA when the segment towards every direction of a 9 x 9 grid over the sun texel (its corners and edges
    included; the texel's directions are the convex hull of its corners' and the wall is convex) meets the wall shrunk by 2 mm, CLEAR when none meets the wall grown by 2 mm,
    and on the penumbra otherwise (left out of both sets; under 15 % of the floor's pixels).  Umbra pixels hold exactly 0.
    The mean of the clear pixels against the twin's rho E / pi, within six of the per-sample std that test_env_ref.py records for the estimator pair, over sqrt(samples):
    with max_bounces = 1 the continuation ray is never traced, so only the NEE half of the pair arrives — its expectation is the integral of L f cos * pdf_env / (pdf_env + P),
    which this test forms by quadrature on the twin and holds the one-bounce frame to; the PAIR, which is what equals rho E / pi (test_env_ref.py (d)), needs the miss of the
    continuation ray and is held to rho E / pi with max_bounces = 2 (the umbra is exactly 0 there too: the wall is black and the floor flat)."""
    rho, spp = 0.5, 64
    c = context(rt, sun_scene(rt), env=sun_map())
    try:
        kw = dict(flags=rt.FLAG_LAMBERT_ONLY, rr_start=2, spp=spp)
        rays, hits = primary_hits(rt, c, **kw)
        prim = hits[:, 3].view(np.uint32)
        floor = np.nonzero(prim < 2)[0]                            # the floor's two triangles come first
        p = rays[floor, 0:3].astype(np.float64) + hits[floor, 0:1].astype(np.float64) * rays[floor, 4:7].astype(np.float64)
        assert np.abs(p[:, 1]).max() < 1e-5
        U, V = np.meshgrid(np.linspace(2 / 8, 3 / 8, 9), np.linspace(5 / 8, 6 / 8, 9))
        D = er.decode_env(U.ravel().astype(np.float32), V.ravel().astype(np.float32))[0].astype(np.float64)
        assert np.abs(D[40] - np.array([-0.64, 0.43, 0.64])).max() < 0.01
        umbra, clear = wall_hits(p, D, -2e-3).all(1), (~wall_hits(p, D, 2e-3)).all(1)
        assert umbra.sum() > 500 and clear.sum() > 1000 and 1.0 - (umbra.sum() + clear.sum()) / len(floor) < 0.15
        # what the clear pixels should hold: E of the sun-only map on a plane facing +Y; and the NEE-only share of it
        tab = er.Tables(sun_map())
        E = er.irradiance_up(sun_map(), 2048)[0]
        x, y, z, w4 = er.grid_rows(2048, np.arange(5 * 256, 6 * 256))
        cols = slice(2 * 256, 3 * 256)
        cosv, pdf = np.maximum(y[:, cols], 0.0), 16.0 * 4.0 / w4[:, cols]            # pmf = 1, N^2 / 4 = 16, r3 = 4 / w4
        nee_only = float((1000.0 * (rho / math.pi) * cosv * (pdf / (pdf + cosv / math.pi)) * w4[:, cols]).sum() / (2048 * 2048))
        pair = rho * E / math.pi
        assert nee_only < pair and abs(float(tab.texels[5, 2, 3]) - 1.0) < 1e-6
        tol = 6.0 * er.SUN_STD / math.sqrt(clear.sum() * spp)
        for bounces, want in ((1, nee_only), (2, pair)):
            img = frame(rt, c, max_bounces=bounces, **kw).reshape(-1, 4)[floor]
            assert (bits(img[umbra, :3]) == 0).all(), bounces
            mean = float((img[clear, 0].astype(np.float64) / spp).mean())
            print(f"sun and blocker, {bounces} bounce(s): clear mean {mean:.4f} against {want:.4f} (pair {pair:.4f}), tolerance {tol:.4f}; umbra {umbra.sum()}, clear {clear.sum()}, floor {len(floor)}")
            assert abs(mean - want) <= tol, bounces
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 7. invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["general", "textured"])
def test_invariance(rt, world, name):
    env = dict(img=world.map64, to_world=world.rot64)
    sc = getattr(world, name)
    c = context(rt, sc, env=env)
    try:
        whole, st = frame(rt, c), c.stats()
        assert st.kernel_launches[rt.K_SHADOW] == 2 * PT["max_bounces"]          # the triangle lights' slot and the environment's
        # two shards rendered in turn
        c.clear(W, H)
        for r in (0, 1):
            c.render(rt.Params(**dict(PT, tile_size=16, shard_rank=r, shard_count=2)))
        assert np.array_equal(bits(c.read_accum()), bits(frame(rt, c, tile_size=16)))
        assert np.array_equal(bits(frame(rt, c, tile_size=16)), bits(whole))
        # adaptive sampling that converges nothing
        c.clear(W, H)
        c.render_adaptive(rt.Params(**PT), 2, 2, PT["spp"], 0.0)
        assert np.array_equal(bits(c.read_accum()), bits(whole))
    finally:
        c.close()
    for opts in ([("OPT_COMPACT_STATE", 0)], [("OPT_GPU_BUILD", 1)]):
        c = context(rt, sc, opts, env=env)
        try:
            assert np.array_equal(bits(frame(rt, c)), bits(whole)), opts
        finally:
            c.close()


# ------------------------------------------------------------------------------------------------
# 8. the state machine
# ------------------------------------------------------------------------------------------------
def test_state_machine_on_a_resident_general_scene(rt, world, tmp_path):
    c = context(rt, world.general)
    try:
        none = frame(rt, c)
        refits, tree = c.stats().bvh_refits, c.tree_hash()
        c.set_environment(world.map8, to_world=world.rot8)
        with pytest.raises(rt.RtxError):                           # rendering between the call and the commit
            c.render(rt.Params(**PT))
        c.commit()
        assert c.stats().bvh_refits == refits and c.tree_hash() == tree      # tables only
        lit = frame(rt, c)
        assert not np.array_equal(bits(lit), bits(none))
        fresh = context(rt, world.general, env=dict(img=world.map8, to_world=world.rot8))      # bound before the first commit
        try:
            assert np.array_equal(bits(frame(rt, fresh)), bits(lit))
        finally:
            fresh.close()
        # invalid arguments leave the scene untouched and committed
        skew = np.eye(4, dtype=np.float32); skew[1, 0] = 0.01
        bad_nan, bad_neg = world.map8.copy(), world.map8.copy()
        bad_nan[3, 3, 1] = np.nan; bad_neg[0, 0, 0] = -1e-3
        for kw in (dict(img=world.map8, to_world=skew.reshape(16)), dict(img=world.map8, scale=-1.0), dict(img=world.map8, scale=float("inf")), dict(img=world.map8, scale=float("nan")),
                   dict(img=bad_nan), dict(img=bad_neg), dict(img=np.zeros((2049, 2049, 3), np.float32)), dict(img=world.map8 * F(1e38), scale=1e38)):
            with pytest.raises(rt.RtxError):
                c.set_environment(**kw)
        assert rt.lib.rtx_set_environment(c._h, world.map8.ctypes.data, 8, None, 1.0, 2) == -1 and rt.lib.rtx_set_environment(c._h, world.map8.ctypes.data, 0, None, 1.0, 0) == -1
        assert np.array_equal(bits(frame(rt, c)), bits(lit))
        # the rejected variants get no copy: the default separate kernels run whatever these say
        for opt in ("OPT_FUSED_BVH", "OPT_SHADE_DENSE", "OPT_SORT_MATERIALS"):
            c.set_option(getattr(rt, opt), 1)
            img, st = frame(rt, c), c.stats()
            assert np.array_equal(bits(img), bits(lit)) and st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] == PT["max_bounces"], opt
            c.set_option(getattr(rt, opt), 0)
        # the scene cache holds no environment
        path = str(tmp_path / "scene.rtxscn")
        with pytest.raises(rt.RtxError):
            c.save_scene_cache(path)
        c.set_environment(None); c.commit()
        assert c.stats().bvh_refits == refits and c.tree_hash() == tree
        assert np.array_equal(bits(frame(rt, c)), bits(none))
        with pytest.raises(rt.RtxError):
            c.env_eval(np.array([[0.0, 1.0, 0.0]], np.float32))
        c.save_scene_cache(path)
        c.set_environment(world.map8); c.commit()
        c.load_scene_cache(path)
        c.set_camera(*world.general.view_proj(W / H))
        assert np.array_equal(bits(frame(rt, c)), bits(none))
        with pytest.raises(rt.RtxError):
            c.env_eval(np.array([[0.0, 1.0, 0.0]], np.float32))
    finally:
        c.close()


def test_state_machine_on_a_tiny_scene(rt, world):
    """a tiny scene runs on the general path while an environment is bound; the commit that crosses the line, either way, is a rebuild; the other render modes ignore it"""
    c = context(rt, world.tiny)
    try:
        kw = dict(flags=rt.FLAG_LAMBERT_ONLY)
        none, st = frame(rt, c, **kw), c.stats()
        assert st.kernel_launches[rt.K_BOUNCE] > 0 and st.kernel_launches[rt.K_SHADE] == 0
        p1 = rt.Params(**dict(PT, spp=1, **kw))
        mesh, o2w = world.tiny.instances[0]
        c.set_instance_transform(0, o2w); c.commit()
        assert c.stats().bvh_refits == 1
        c.set_environment(np.zeros((4, 4, 3), np.float32)); c.commit()      # bound, even a black one
        assert c.stats().bvh_refits == 0
        img, st = frame(rt, c, **kw), c.stats()
        assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] == PT["max_bounces"]
        assert np.allclose(img, none, rtol=1e-3, atol=1e-3)         # (the two paths agree by the parity contract, which other tests hold; a black map adds nothing)
        c.clear(W, H); c.render_v6_pass1(p1); pass1 = c.read_accum()
        c.set_environment(np.full((4, 4, 3), 0.25, np.float32)); c.commit()
        lit = frame(rt, c, **kw)
        assert lit[..., :3].sum() > none[..., :3].sum()
        c.clear(W, H); c.render_v6_pass1(p1)
        assert np.array_equal(bits(c.read_accum()), bits(pass1))    # pass 1 ignores the environment
        c.set_instance_transform(0, o2w); c.commit()
        assert c.stats().bvh_refits == 1
        c.set_environment(None); c.commit()
        assert c.stats().bvh_refits == 0
        img, st = frame(rt, c, **kw), c.stats()
        assert st.kernel_launches[rt.K_BOUNCE] > 0 and st.kernel_launches[rt.K_SHADE] == 0 and np.array_equal(bits(img), bits(none))
    finally:
        c.close()


# ------------------------------------------------------------------------------------------------
# 9. the command line
# ------------------------------------------------------------------------------------------------
def test_cli_environment(rt, world, tmp_path):
    exe = os.path.join(graft.PKG_DIR, "rtx_render")
    rng = np.random.default_rng(9)
    latlong = rng.uniform(0.0, 2.0, (24, 48, 3)).astype(np.float32)
    latlong[4:7, 30:34] = 40.0
    (tmp_path / "sky.pfm").write_bytes(pfm_bytes(latlong, True))
    base = [exe, "--scene", "cornell", "--w", str(W), "--h", str(H), "--spp", "4"]

    def run(args, out):
        r = subprocess.run(base + args + ["--out", str(tmp_path / out)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(str(tmp_path / out))

    def own(**env):
        c = context(rt, world.tiny, env=env)
        try:
            a = frame(rt, c, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=rt.FLAG_LAMBERT_ONLY)
            return a[..., :3] / np.maximum(a[..., 3:4], F(1.0))
        finally:
            c.close()

    px = run(["--env", str(tmp_path / "sky.pfm"), "--env-res", "16"], "env.exr")
    assert np.array_equal(bits(px), bits(own(img=rt.latlong_to_octahedral(latlong, 16))))
    assert not np.array_equal(bits(px), bits(run([], "none.exr")))
    sky = run(["--sky", "0.5,0.7,1.0"], "sky.exr")
    assert np.array_equal(bits(sky), bits(own(img=np.array([[[0.5, 0.7, 1.0]]], np.float32))))
    two = run(["--env", str(tmp_path / "sky.pfm"), "--env-res", "16", "--gpus", "2", "--devices", "0,0", "--gather", "copy"], "two.exr")
    assert np.array_equal(bits(two), bits(px))
    turned = run(["--env", str(tmp_path / "sky.pfm"), "--env-res", "16", "--env-yaw", "90", "--env-scale", "2", "--env-hidden"], "turned.exr")
    ang = 90.0 * 3.14159265358979323846 / 180.0                  # (as the command line forms it)
    cs, sn = F(math.cos(ang)), F(math.sin(ang))
    m = np.eye(4, dtype=np.float32).reshape(16); m[0], m[8], m[2], m[10] = cs, sn, -sn, cs
    assert np.array_equal(bits(turned), bits(own(img=rt.latlong_to_octahedral(latlong, 16), to_world=m, scale=2.0, hidden=True)))
    r = subprocess.run(base + ["--env", str(tmp_path / "missing.hdr")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "missing.hdr" in r.stderr

"""Emission maps on the device (include/rtx.h: EMISSION MAPS): the two probes and rtx_get_lights against the numpy twin (tests/emimap_ref.py) bit for bit; consequence (a) —
a scene whose mapped emitter triangles each see one texel value against the unmapped scene that carries one material per value — as whole frames, bit for bit and with equal
ray counts, over the kernels the flag reaches; consequence (b); the things that ignore the map; consequence (c), the one statistical test; the commit rules; the tiny-scene
line; the command line.  Frames are 64 x 32 (several 256-entry queue chunks, partial waves at late bounces), at most 16 spp, 1 - 3 bounces."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import emimap_ref as em
import texture_ref as tr
from test_deform import ArrayScene, bits, random_rays
from test_specmap import camera, grid, join, material, tri_tables

W, H = 64, 32
PT = dict(width=W, height=H, spp=4, max_bounces=3, nee_samples=1, rr_start=2)
MISS = np.uint32(0xFFFFFFFF)
ERR_INVALID, ERR_STATE = -1, -4
F = np.float32
EYE = np.eye(4, dtype=np.float32).reshape(16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class EmiScene(ArrayScene):
    """ArrayScene + the texture attributes Context.upload binds"""
    def __init__(self, base, uvs, textures, ke=None, environment=None, materials=None, meshes=None):
        super().__init__(base.materials if materials is None else materials, base.meshes if meshes is None else meshes, base.instances, base._vp, base.lo, base.hi)
        self.uvs, self.textures, self.ke_maps = uvs, textures, ke
        if environment is not None:
            self.environment = environment


def based(part, base):
    """a grid()'s mesh with Vertex.normal.w = the mesh's offset in the scene's material ids"""
    v, i, m, uv = part
    v = v.copy(); v[:, 6] = float(base)
    return (v, i, m), uv


def context(rt, opts, scene):
    c = rt.Context(0)
    for o, v in opts:
        c.set_option(getattr(rt, o), v)
    c.upload(scene, W / H)
    return c


def frame(rt, c, flags=0, **kw):
    c.clear(W, H)
    c.render(rt.Params(flags=flags, **dict(PT, **kw)))
    return c.read_accum()


def rays_of(st):
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def general_path(rt, st):
    return st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] > 0


# ------------------------------------------------------------------------------------------------
# 1: the probes and the light records against the twin, bit for bit
# ------------------------------------------------------------------------------------------------
P_WALL_A, P_WALL_B, P_SIGN, P_SCREEN, P_LAMP = range(5)      # materials: two walls (B has an emission map bound: no effect); an emitter mapped through an sRGB 5 x 3 texture; one
                                                             # through a linear 7 x 4 with black texels; an unmapped emitter


class ProbeWorld:
    """a 4 x 3 x 4 room of 2 x 2 quads per face (48 triangles, one mesh) and three emitter meshes of 2 x 2 quads: the sign (one instance), the screen (two instances, one of
    them mirrored and scaled) and the lamp: 80 triangles, UVs from -0.7 to 1.8"""
    def __init__(self, rt):
        rng = np.random.default_rng(20261024)
        self.materials = np.stack([material(rt, (0.7, 0.6, 0.5), (0.4, 0.4, 0.4), 0.6, 0.1), material(rt, (0.3, 0.6, 0.7), (0.5, 0.5, 0.5), 0.9, 0.2),
                                   material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(12, 11.3, 9.7)), material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(3.1, 6.2, 9.3)),
                                   material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(5, 5, 4))])
        faces = [((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0)), ((-2, 3, -2), (0, 0, 4), (4, 0, 0), (0, -1, 0)), ((-2, 0, -2), (0, 3, 0), (4, 0, 0), (0, 0, 1)),
                 ((-2, 0, 2), (4, 0, 0), (0, 3, 0), (0, 0, -1)), ((-2, 0, -2), (0, 0, 4), (0, 3, 0), (1, 0, 0)), ((2, 0, -2), (0, 3, 0), (0, 0, 4), (-1, 0, 0))]
        wide = lambda q, a, b: [(q % 2 + a) / 2 * 2.5 - 0.7, (q // 2 + b) / 2 * 2.5 - 0.7]
        room = join([grid(o, dv, du, 2, 2, n, [(P_WALL_A, P_WALL_B)[(f + q) % 2] for q in range(4)], wide) for f, (o, du, dv, n) in enumerate(faces)])
        sign = grid((-1.5, 2.75, -1.5), (1.0, 0, 0), (0, 0, 1.0), 2, 2, (0, -1, 0), [P_SIGN] * 4, wide)
        screen = grid((0.25, 2.5, -0.5), (0.75, 0, 0), (0, 0, 0.75), 2, 2, (0, -1, 0), [P_SCREEN] * 4, wide)
        lamp = grid((-0.5, 2.875, -0.25), (0.75, 0, 0), (0, 0, 1.0), 2, 2, (0, -1, 0), [P_LAMP] * 4, wide)
        self.meshes, self.uvs, base = [], [], 0
        for part in (room, sign, screen, lamp):
            mesh, uv = based(part, base)
            self.meshes.append(mesh); self.uvs.append(uv); base += len(mesh[1])
        mirror = np.eye(4, dtype=np.float32); mirror[0, 0] = -1.5; mirror[3, 0] = 0.25; mirror[3, 1] = -0.5; mirror[3, 2] = -1.0      # x -> 0.25 - 1.5 x: mirrored, scaled, lower
        self.instances = [(0, EYE), (1, EYE), (2, EYE), (2, mirror.reshape(16)), (3, EYE)]
        self.plain = ArrayScene(self.materials, self.meshes, self.instances, camera(rt, (0.0, 0.4, 1.9), (0.0, 1.9, -0.6), (0, 1, 0), 80.0), -1.9, 1.9)
        screen_px = rng.integers(0, 256, (4, 7, 4), dtype=np.uint8); screen_px[1:3, 2:5, :3] = 0; screen_px[0, 0, 1] = 0
        self.textures = [(rng.integers(0, 256, (3, 5, 4), dtype=np.uint8), True), (screen_px, False)]
        self.ke = [-1, 0, 0, 1, -1]
        self.mapped = EmiScene(self.plain, self.uvs, self.textures, self.ke)
        self.unmapped = EmiScene(self.plain, self.uvs, self.textures)
        self.tri_mat, self.tri_uv = tri_tables(self.meshes, self.uvs, self.instances)
        self.lights = em.LightList(rt.half_round, self.materials, self.meshes, self.uvs, self.instances, self.textures, self.ke)
        self.lights_unmapped = em.LightList(rt.half_round, self.materials, self.meshes, self.uvs, self.instances, self.textures, None)


@pytest.fixture(scope="module")
def probe_world(rt):
    return ProbeWorld(rt)


def probe_hits(rt, c, w):
    rays = np.concatenate([c.primary_rays(rt.Params(**PT)), random_rays(6000, 7, w.plain.lo, w.plain.hi)])
    rays[:, 1] = np.clip(rays[:, 1], 0.1, 2.4)                               # (origins inside the room, below the emitters)
    rays[-20:, 0:3] = (50.0, 50.0, 50.0); rays[-20:, 4:7] = (0.0, 1.0, 0.0)   # ... and a few that miss
    return c.trace_closest(rays)


@pytest.mark.gpu
def test_emission_probe_equals_the_twin(rt, probe_world):
    w = probe_world
    c = context(rt, [], w.mapped)
    assert c.stats().triangles == 80 == len(w.tri_mat) and w.lights.active
    hits = probe_hits(rt, c, w)
    want_v, want_t = em.emission_probe(rt.half_round, w.textures, w.ke, w.materials, w.lights.q, w.tri_mat, w.tri_uv, hits)
    got_v, got_t = c.emission(hits)
    assert len(hits) >= 5000 and np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_t, want_t)
    prim = hits[:, 3].copy().view(np.uint32); hit = prim != MISS
    mat = w.tri_mat[np.where(hit, prim, 0)]
    for m in range(5):
        assert (hit & (mat == m)).sum() > 20, m
    s, t = tr.interp_uv(w.tri_uv[np.where(hit, prim, 0)], hits[:, 1], hits[:, 2])
    on = hit & (mat >= P_SIGN)
    assert (s[on] < 0).any() and (s[on] > 1).any() and (t[on] < 0).any() and (t[on] > 1).any()              # the wrap is exercised on the emitters
    ke_tab = tr.half_round_array(rt.half_round, w.materials[:, 8:11])
    sel = hit & (mat == P_SIGN); assert (got_t[sel] == 0).all() and (bits(got_v[sel, :3]) != bits(ke_tab[P_SIGN])).any() and (got_v[sel, 3] > 0).all()
    sel = hit & (mat == P_SCREEN); assert (got_t[sel] == 1).all() and (got_v[sel, :3] == 0).all(axis=1).any() and (got_v[sel, :3] > 0).any()      # black texels: Ke' = 0, still an emitter
    sel = hit & (mat == P_LAMP); assert (got_t[sel] == MISS).all() and np.array_equal(bits(got_v[sel, :3]), bits(ke_tab[mat[sel]]))
    assert np.array_equal(bits(got_v[sel, 3]), bits(np.repeat(((ke_tab[P_LAMP, 0] + ke_tab[P_LAMP, 1]) + ke_tab[P_LAMP, 2]) / F(3.0), sel.sum())))
    sel = hit & (mat <= P_WALL_B); assert not got_v[sel].any() and (got_t[sel] == MISS).all()               # a map on a non-emitter: nothing
    assert (~hit).sum() >= 20 and not got_v[~hit].any() and (got_t[~hit] == MISS).all()
    # q differs between the instances of one mesh only through... nothing: the table depends on no transform
    q = w.lights.q; assert np.array_equal(bits(q[56:64]), bits(q[64:72])) and (q[:48] == 0).all()
    assert rt.lib.rtx_debug_emission(c._h, None, 1, None) == ERR_INVALID
    c.close()
    c = context(rt, [], w.unmapped)                                          # no emission map active: the table's Ke and its mean, no texture
    want_v, want_t = em.emission_probe(rt.half_round, w.textures, None, w.materials, None, w.tri_mat, w.tri_uv, hits, active=False)
    got_v, got_t = c.emission(hits)
    assert np.array_equal(bits(got_v), bits(want_v)) and (got_t == MISS).all() and (got_v[hit & (mat == P_SIGN), 3] > 0).all()
    c.close()


@pytest.mark.gpu
def test_light_sample_probe_and_light_records_equal_the_twin(rt, probe_world):
    w = probe_world
    rng = np.random.default_rng(12)
    seeds = rng.integers(0, 2 ** 32, (6000, 2), dtype=np.uint64).astype(np.uint32)
    for scene, L, active in ((w.mapped, w.lights, True), (w.unmapped, w.lights_unmapped, False)):
        c = context(rt, [], scene)
        assert c.stats().lights == 32 == len(L.records)
        assert np.array_equal(bits(c.lights()), bits(L.records)), active    # rtx_get_lights: layout and em kept, weights, order and CDF the twin's
        got = c.light_sample(seeds)
        want = em.light_sample(L, w.textures, w.tri_uv, seeds, active)
        assert np.array_equal(got["light"], want["light"]) and np.array_equal(got["seed"], want["seed"]), active
        for k in ("point", "st", "em", "pdf_l"):
            assert np.array_equal(bits(got[k]), bits(want[k])), (k, active)
        assert len(np.unique(got["light"])) >= (24 if active else 32)       # (mapped: triangles under black texels carry little or no weight)
        if active:
            tex = L.tex[got["light"]]
            assert set(tex.tolist()) == {0, 1, -1} and not got["st"][tex < 0].any() and (got["st"][tex >= 0] != 0).any()
            rec = L.records[got["light"], 12:15]
            assert (bits(got["em"][tex >= 0]) != bits(rec[tex >= 0])).any() and np.array_equal(bits(got["em"][tex < 0]), bits(rec[tex < 0]))
            assert (got["em"][tex == 1] == 0).all(axis=1).any()              # a sample on a black texel: a zero contribution, no shadow ray
        c.close()
    assert not np.array_equal(w.lights.prim, w.lights_unmapped.prim) and sorted(w.lights.prim.tolist()) == sorted(w.lights_unmapped.prim.tolist())      # only weights and order change


# ------------------------------------------------------------------------------------------------
# 2: consequence (a) — whole frames, bit for bit
# ------------------------------------------------------------------------------------------------
NB, BLK = 4, 4                                                            # the block textures: NB x NB blocks of BLK x BLK texels, one value per block
G_FLOOR, G_WALL, G_SIGN_A, G_SIGN_B = range(4)                            # base materials


def block_texture(rng):
    vals = rng.integers(1, 256, (NB, NB, 4), dtype=np.uint8)                 # every component of every block's value > 0
    return np.repeat(np.repeat(vals, BLK, axis=0), BLK, axis=1)


def block_uv(q, a, b):
    """quad q lies inside the interior of block (q % NB, q // NB): texel columns [4 i + 1, 4 i + 3] of 16, where all four taps of Sample read the block's value"""
    i, j = q % NB, (q // NB) % NB
    n = NB * BLK
    return [(BLK * i + 1 + 2 * a) / n, 1.0 - (BLK * j + 3 - 2 * b) / n]


class GridWorld:
    """a 4 x 4 grid of emitter quads under the ceiling (32 triangles, two materials in a checkerboard, each with its own block texture), a floor of 4 x 4 quads and a back
    wall of 2 x 2: 72 triangles, so that the mapped and the unmapped scene both run the general path"""
    def __init__(self, rt):
        rng = np.random.default_rng(20261025)
        self.rt = rt
        self.materials = np.stack([material(rt, (0.6, 0.55, 0.5), (0.6, 0.6, 0.6), 0.5, 0.3), material(rt, (0.4, 0.5, 0.6), (0.5, 0.5, 0.5), 0.9, 0.1),
                                   material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(10, 8.3, 6.1)), material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(3.3, 5.7, 7.9))])
        signs = grid((-1.5, 2.5, -1.5), (3, 0, 0), (0, 0, 3), 4, 4, (0, -1, 0), [(G_SIGN_A, G_SIGN_B)[(q + q // 4) % 2] for q in range(16)], block_uv)
        floor = grid((-2, 0, -2), (0, 0, 4), (4, 0, 0), 4, 4, (0, 1, 0), [G_FLOOR] * 16, block_uv)       # (du x dv = the side the flat normal faces)
        wall = grid((-2, 0, -2), (4, 0, 0), (0, 3, 0), 2, 2, (0, 0, 1), [G_WALL] * 4, block_uv)
        v, i, m, uv = join([signs, floor, wall])
        self.meshes, self.uvs = [(v, i, m)], [uv]
        self.instances = [(0, EYE)]
        self.plain = ArrayScene(self.materials, self.meshes, self.instances, camera(rt, (0.0, 0.5, 2.6), (0.0, 1.4, -1.0), (0, 1, 0), 75.0), -1.9, 1.9)
        self.textures = [(block_texture(rng), True), (block_texture(rng), False)]
        self.ke = [-1, -1, 0, 1]
        self.tri_mat, self.tri_uv = tri_tables(self.meshes, self.uvs, self.instances)

    def mapped(self, env=None, ke=None, textures=None):
        return EmiScene(self.plain, self.uvs, self.textures if textures is None else textures, self.ke if ke is None else ke, env)

    def unmapped(self, env=None):
        return EmiScene(self.plain, self.uvs, self.textures, None, env)

    def unmapped_equivalent(self, env=None):
        """the scene of consequence (a): no emission map, one material per emitter quad with Ke = KeFull * c (a float32 product), c the quad's texel value"""
        for tex in range(2):                                                 # the premise: every emitter triangle's taps agree, at its corners and inside
            for uv in (self.tri_uv[:32, 0], self.tri_uv[:32, 1], self.tri_uv[:32, 2], self.tri_uv[:32].mean(axis=1)):
                assert tr.taps_agree(self.textures[tex][0], uv[:, 0], uv[:, 1]).all()
        mats, tri_new = [m for m in self.materials[:2]], self.tri_mat.astype(np.uint32).copy()
        for q in range(16):
            base = int(self.tri_mat[2 * q]); tex = self.ke[base]
            mid = self.tri_uv[2 * q].mean(axis=0)
            c = tr.sample(self.textures[tex][0], self.textures[tex][1], mid[:1], mid[1:2])[0]
            assert (c > 0).all()
            m = self.materials[base].copy(); m[8:11] = m[8:11] * c
            tri_new[2 * q:2 * q + 2] = len(mats); mats.append(m)
        v, i, _ = self.meshes[0]
        return EmiScene(self.plain, self.uvs, self.textures, None, env, materials=np.stack(mats), meshes=[(v, i, np.repeat(tri_new, 3))])


@pytest.fixture(scope="module")
def grid_world(rt):
    return GridWorld(rt)


@pytest.mark.gpu
@pytest.mark.parametrize("lambert", [False, True])
@pytest.mark.parametrize("with_env", [False, True])
def test_constant_blocks_are_the_unmapped_scene_with_more_materials(rt, grid_world, lambert, with_env):
    w = grid_world
    env = np.random.default_rng(4).uniform(0.0, 1.5, (8, 8, 3)).astype(np.float32) if with_env else None
    a, b = w.mapped(env), w.unmapped_equivalent(env)
    assert len(b.materials) == 18 and len(a.materials) == 4
    flags = rt.FLAG_LAMBERT_ONLY if lambert else 0
    for compact in (1, 0):
        ctxs = [context(rt, [("OPT_COMPACT_STATE", compact)], sc) for sc in (a, b)]
        la, lb = ctxs[0].lights(), ctxs[1].lights()                       # the same list — corners, instance, CDF, weights, total — but for em: the material's Ke on each side
        assert np.array_equal(bits(la[:, :12]), bits(lb[:, :12])) and np.array_equal(bits(la[:, 15:]), bits(lb[:, 15:])) and not np.array_equal(bits(la[:, 12:15]), bits(lb[:, 12:15]))
        for nee in (1, 2):
            imgs, stats = [], []
            for c in ctxs:
                assert c.stats().triangles == 72
                imgs.append(frame(rt, c, flags, nee_samples=nee)); st = c.stats()
                stats.append(rays_of(st))
                assert general_path(rt, st)
            assert imgs[0][..., :3].sum() > 0 and np.isfinite(imgs[0]).all() and np.array_equal(bits(imgs[0]), bits(imgs[1])), (compact, nee)
            assert stats[0] == stats[1] and stats[0][2] > 0, (compact, nee)
        ids = ctxs[0].emission(ctxs[0].trace_closest(ctxs[0].primary_rays(rt.Params(**PT))))[1]
        assert (ids == 0).sum() > 30 and (ids == 1).sum() > 30               # the camera sees both kinds of sign: the emissive hit's look-up ran at bounce 0 too
        for c in ctxs:
            c.close()


@pytest.mark.gpu
def test_constant_blocks_under_adaptive_sampling(rt, grid_world):
    w = grid_world
    out = []
    for sc in (w.mapped(), w.unmapped_equivalent()):
        c = context(rt, [], sc)
        c.clear(W, H)
        res = c.render_adaptive(rt.Params(**PT), 4, 4, 12, 0.05)
        out.append((c.read_accum(), (res.passes, res.chunks_converged, res.chunks_at_max, res.pixel_samples), rays_of(c.stats())))
        c.close()
    assert out[0][0][..., :3].sum() > 0 and np.array_equal(bits(out[0][0]), bits(out[1][0])) and out[0][1:] == out[1][1:]


# ------------------------------------------------------------------------------------------------
# 3: consequence (b), a map on a non-emitter, and who ignores the map
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("lambert", [False, True])
def test_all_255_map_changes_nothing(rt, grid_world, lambert):
    w = grid_world
    white = [(np.full((5, 3, 4), 255, np.uint8), False)]
    flags = rt.FLAG_LAMBERT_ONLY if lambert else 0
    imgs, stats, recs = [], [], []
    for sc in (w.mapped(ke=[-1, -1, 0, 0], textures=white), w.unmapped()):
        c = context(rt, [], sc)
        imgs.append(frame(rt, c, flags)); stats.append(rays_of(c.stats())); recs.append(c.lights())
        ids = c.emission(c.trace_closest(c.primary_rays(rt.Params(**PT))))[1]
        assert (ids != MISS).any() == (sc.ke_maps is not None)               # the map is ACTIVE on the first side: k_shade's emission-mapped form runs there
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1])) and stats[0] == stats[1] and np.array_equal(bits(recs[0]), bits(recs[1]))


@pytest.mark.gpu
def test_a_map_on_a_non_emitter_changes_nothing(rt, grid_world):
    w = grid_world
    imgs, stats, launches = [], [], []
    for sc in (w.mapped(ke=[0, 1, -1, -1]), w.unmapped()):
        c = context(rt, [], sc)
        imgs.append(frame(rt, c)); st = c.stats()
        stats.append(rays_of(st)); launches.append(list(st.kernel_launches))
        assert (c.emission(c.trace_closest(c.primary_rays(rt.Params(**PT))))[1] == MISS).all()
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1])) and stats[0] == stats[1] and launches[0] == launches[1]


@pytest.mark.gpu
def test_pass1_restir_and_the_denoiser_ignore_the_map(rt, grid_world):
    w = grid_world
    p1 = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=4, flags=0, frame_seed=5)
    out = []
    for sc in (w.mapped(), w.unmapped()):
        c = context(rt, [], sc)
        got = {"frame": frame(rt, c), "layer16": c.read_layer(16, W, H), "guides": c.denoise_guides(W, H)}
        c.clear(W, H); c.render_v6_pass1(p1); got["pass1"] = c.read_accum()
        c.denoise(W, H, 3); got["denoised"] = c.read_denoised()                # (of the pass-1 frame, which the map does not reach: emitters pass through as ever)
        vp = sc.view_proj(W / H)
        c.set_camera(*vp); c.set_camera(*vp); c.restir_reset()                # previous view = current view
        c.clear(W, H); c.render_restir(rt.Params(**dict(PT, spp=2, max_bounces=3, nee_samples=4))); got["restir"] = c.read_accum()
        out.append(got); c.close()
    for k in ("layer16", "guides", "pass1", "denoised", "restir"):
        assert np.array_equal(out[0][k].view(np.uint8), out[1][k].view(np.uint8)), k
    assert out[0]["pass1"][..., :3].sum() > 0 and out[0]["restir"][..., :3].sum() > 0
    assert not np.array_equal(bits(out[0]["frame"]), bits(out[1]["frame"]))  # ... and rtx_render does see it


# ------------------------------------------------------------------------------------------------
# 4: consequence (c) — unbiased whatever the quadrature misses: NEE-heavy and BSDF-heavy estimates of one image agree
# ------------------------------------------------------------------------------------------------
class SpotWorld:
    """a diffuse floor (2 x 2 quads) under one emitter quad whose 16 x 16 map is a bright 2 x 2-texel spot on black: 10 triangles"""
    def __init__(self, rt):
        self.materials = np.stack([material(rt, (0.7, 0.7, 0.7), (0.3, 0.3, 0.3), 0.7, 0.0), material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(60, 50, 40))])
        full = lambda q, a, b: [a, b]
        floor = grid((-4, 0, -3), (0, 0, 6), (8, 0, 0), 2, 2, (0, 1, 0), [0] * 4, lambda q, a, b: [0.0, 0.0])
        lamp = grid((-1, 1.0, -1), (2, 0, 0), (0, 0, 2), 1, 1, (0, -1, 0), [1], full)
        v, i, m, uv = join([floor, lamp])
        self.meshes, self.uvs, self.instances = [(v, i, m)], [uv], [(0, EYE)]
        self.plain = ArrayScene(self.materials, self.meshes, self.instances, camera(rt, (0.0, 2.2, 3.4), (0.0, 0.0, -0.2), (0, 1, 0), 50.0), -1.9, 1.9)
        spot = np.zeros((16, 16, 4), np.uint8); spot[7:9, 7:9, :3] = 255
        self.spot = EmiScene(self.plain, self.uvs, [(spot, False)], [-1, 0])
        self.white = EmiScene(self.plain, self.uvs, [(np.full((16, 16, 4), 255, np.uint8), False)], [-1, 0])


def block_means(img):
    """(H, W, 3) -> (H / 4, W / 4, 3): the mean of every 4 x 4-pixel block"""
    return img.reshape(H // 4, 4, W // 4, 4, 3).mean(axis=(1, 3))


@pytest.mark.gpu
def test_nee_and_bsdf_sampling_agree_under_a_spot_map(rt):
    """32 frames x 16 spp per side, 2 bounces, GGX; the measured standard errors and the shadow-ray shares are recorded in profiles/emimap_energy.md"""
    w = SpotWorld(rt)
    frames, spp, mb = 32, 16, 2
    c = context(rt, [], w.spot)
    prim = c.trace_closest(c.primary_rays(rt.Params(**PT)))[:, 3].copy().view(np.uint32).reshape(H, W)
    on_floor = (prim < 8).reshape(H // 4, 4, W // 4, 4).all(axis=(1, 3))      # blocks whose 16 pixels all see the floor first
    assert on_floor.sum() >= 40
    L = em.LightList(rt.half_round, w.materials, w.meshes, w.uvs, w.instances, w.spot.textures, w.spot.ke_maps)
    assert np.array_equal(bits(c.lights()), bits(L.records)) and (L.q[8:] > 0).all() and (L.q[:8] == 0).all()
    means = {}
    for nee in (1, 4):
        per_frame = []
        for f in range(frames):
            c.clear(W, H)
            c.render(rt.Params(width=W, height=H, spp=spp, sample_base=1 + f * spp, max_bounces=mb, nee_samples=nee, rr_start=mb, frame_seed=1 + f + 100 * nee, flags=0))
            a = c.read_accum()
            assert (a[..., 3] == spp).all()
            per_frame.append(block_means(a[..., :3].astype(np.float64) / spp)[on_floor])
        per_frame = np.array(per_frame)
        means[nee] = (per_frame.mean(axis=0), per_frame.std(axis=0, ddof=1) / np.sqrt(frames))
        if nee == 1:
            st = c.stats(); share_spot = st.rays_shadow / st.kernel_items[rt.K_SHADE]
            assert general_path(rt, st)
    c.close()
    (m1, se1), (m4, se4) = means[1], means[4]
    se = np.sqrt(se1 ** 2 + se4 ** 2)
    lit = se > 0
    ratio = np.abs(m1 - m4)[lit] / se[lit]
    print(f"spot map: {on_floor.sum()} floor blocks x 3 channels, {frames} frames x {spp} spp; block mean {m1.mean():.4f} (nee 1) {m4.mean():.4f} (nee 4); standard error of a block mean: "
          f"median {np.median(se1):.5f} max {se1.max():.5f} (nee 1), median {np.median(se4):.5f} max {se4.max():.5f} (nee 4); largest |difference| / standard error of the difference {ratio.max():.2f}")
    assert lit.mean() > 0.9 and m1.mean() > 0.01
    assert (np.abs(m1 - m4) <= 6.0 * se).all(), float(ratio.max())
    # the share of NEE shadow rays per shaded hit falls against an all-255 map: black triangles and zero contributions ask for no shadow ray
    c = context(rt, [], w.white)
    c.clear(W, H); c.render(rt.Params(width=W, height=H, spp=spp, sample_base=1 + (frames - 1) * spp, max_bounces=mb, nee_samples=1, rr_start=mb, frame_seed=frames + 100, flags=0))
    st = c.stats(); share_white = st.rays_shadow / st.kernel_items[rt.K_SHADE]
    c.close()
    print(f"shadow rays per shaded hit: {share_spot:.4f} with the spot map, {share_white:.4f} with the all-255 map, ratio {share_spot / share_white:.3f}")
    assert share_spot < share_white


# ------------------------------------------------------------------------------------------------
# 5: commits, state, errors
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_commit_rules_and_errors(rt, grid_world, tmp_path):
    w = grid_world
    L = rt.lib
    c = context(rt, [], w.mapped())
    p = rt.Params(**PT)
    ref = frame(rt, c)
    refits, tree, lights = c.stats().bvh_refits, c.tree_hash(), c.lights()
    hits = c.trace_closest(c.primary_rays(p))
    # slot 11 is no slot, slot 12 is one; invalid calls leave the committed scene untouched: the next frame's bits are equal
    for slot in (11, 13, 14):
        assert L.rtx_set_material_map(c._h, G_SIGN_A, slot, 0) == ERR_INVALID, slot
    assert L.rtx_set_material_map(c._h, len(w.materials), rt.MAP_KE, 0) == ERR_INVALID and L.rtx_set_material_map(c._h, G_SIGN_A, rt.MAP_KE, len(w.textures)) == ERR_INVALID
    assert L.rtx_set_material_map(c._h, G_SIGN_A, rt.MAP_KE, -2) == ERR_INVALID
    assert np.array_equal(bits(frame(rt, c)), bits(ref))                     # (still committed: no RTX_ERR_STATE)
    # rtx_save_scene_cache with an emission map bound
    assert L.rtx_save_scene_cache(c._h, str(tmp_path / "s.rtxscn").encode()) == ERR_STATE
    # a map call opens the RTX_ERR_STATE window; the map-only commit rebuilds the light list and leaves the tree alone
    assert L.rtx_set_material_map(c._h, G_SIGN_A, 12, 1) == 0
    assert L.rtx_render(c._h, ctypes.byref(p)) == ERR_STATE                  # rendering before the commit
    c.commit()
    assert (c.stats().bvh_refits, c.tree_hash()) == (refits, tree) and c.stats().lights == 32
    want = em.LightList(rt.half_round, w.materials, w.meshes, w.uvs, w.instances, w.textures, [-1, -1, 1, 1])
    assert np.array_equal(bits(c.lights()), bits(want.records)) and not np.array_equal(want.prim, em.LightList(rt.half_round, w.materials, w.meshes, w.uvs, w.instances, w.textures, w.ke).prim)
    assert not np.array_equal(bits(frame(rt, c)), bits(ref))
    # ... and so does a commit after rtx_set_texture alone, and after rtx_set_mesh_uvs alone
    c.set_texture(1, w.textures[1][0][::-1].copy(), False)
    assert L.rtx_render(c._h, ctypes.byref(p)) == ERR_STATE
    c.commit()
    flipped = [w.textures[0], (w.textures[1][0][::-1].copy(), False)]
    want = em.LightList(rt.half_round, w.materials, w.meshes, w.uvs, w.instances, flipped, [-1, -1, 1, 1])
    assert np.array_equal(bits(c.lights()), bits(want.records)) and (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    uv2 = w.uvs[0][::-1].copy()
    c.set_mesh_uvs(0, uv2); c.commit()
    want = em.LightList(rt.half_round, w.materials, w.meshes, [uv2], w.instances, flipped, [-1, -1, 1, 1])
    assert np.array_equal(bits(c.lights()), bits(want.records)) and (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    got_v, _ = c.emission(hits)
    want_v, _ = em.emission_probe(rt.half_round, flipped, [-1, -1, 1, 1], w.materials, want.q, w.tri_mat, uv2.reshape(-1, 3, 2), hits)
    assert np.array_equal(bits(got_v), bits(want_v))                         # the q table followed too
    # back to the first state: the first frame, to the bit
    c.set_mesh_uvs(0, w.uvs[0]); c.set_texture(1, w.textures[1][0], False); c.set_material_map(G_SIGN_A, 0, rt.MAP_KE); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(ref)) and np.array_equal(bits(c.lights()), bits(lights)) and (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    # unbinding the last map is the commit after which none is active: the unmapped list and frame
    c.set_material_map(G_SIGN_A, None, rt.MAP_KE); c.set_material_map(G_SIGN_B, None, rt.MAP_KE); c.commit()
    q = context(rt, [], w.unmapped())
    plain, plain_lights = frame(rt, q), q.lights()
    q.close()
    assert np.array_equal(bits(frame(rt, c)), bits(plain)) and np.array_equal(bits(c.lights()), bits(plain_lights)) and (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    assert (c.emission(hits)[1] == MISS).all()
    # rtx_set_materials resets the slot
    c.set_material_map(G_SIGN_A, 0, rt.MAP_KE); c.set_material_map(G_SIGN_B, 1, rt.MAP_KE); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(ref)) and (c.emission(hits)[1] != MISS).any()
    c.set_materials(w.materials); c.commit()
    assert (c.emission(hits)[1] == MISS).all() and np.array_equal(bits(frame(rt, c)), bits(plain)) and np.array_equal(bits(c.lights()), bits(plain_lights))
    # a transform-only commit of a mapped scene: a refit, the same weights and q (the table depends on no transform)
    c.set_material_map(G_SIGN_A, 0, rt.MAP_KE); c.set_material_map(G_SIGN_B, 1, rt.MAP_KE); c.commit()
    before = c.stats().bvh_refits
    move = EYE.copy(); move[13] = 0.125
    c.set_instance_transform(0, move); c.commit()
    moved = c.lights()
    assert c.stats().bvh_refits == before + 1 and np.array_equal(bits(moved[:, 11]), bits(lights[:, 11])) and np.array_equal(bits(moved[:, 3]), bits(lights[:, 3]))
    assert np.array_equal(bits(c.emission(hits)[0]), bits(em.emission_probe(rt.half_round, w.textures, w.ke, w.materials,
                          em.LightList(rt.half_round, w.materials, w.meshes, w.uvs, w.instances, w.textures, w.ke).q, w.tri_mat, w.tri_uv, hits)[0]))
    c.close()


@pytest.mark.gpu
def test_an_all_black_map_leaves_no_light_list(rt, grid_world):
    """every emitter's map black: total weight 0, no NEE slots, the random numbers of a scene without lights — the frame with nee_samples = 1 is the frame with
    nee_samples = 0, to the bit, under an environment that lights it; the count of lights stays"""
    w = grid_world
    env = np.random.default_rng(4).uniform(0.0, 1.5, (8, 8, 3)).astype(np.float32)
    black = [(np.zeros((4, 4, 4), np.uint8), False)]
    c = context(rt, [], w.mapped(env, ke=[-1, -1, 0, 0], textures=black))
    imgs, stats = [], []
    for nee in (1, 0, 2):
        imgs.append(frame(rt, c, nee_samples=nee)); stats.append(rays_of(c.stats()))
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1])) and np.array_equal(bits(imgs[0]), bits(imgs[2])) and stats[0] == stats[1] == stats[2]
    assert c.stats().lights == 32 and len(c.lights()) == 32 and not c.lights()[:, 11].any() and c.lights()[0, 16] == 0
    assert rt.lib.rtx_debug_light_sample(c._h, None, 0, None) == ERR_STATE
    ke, ids = c.emission(c.trace_closest(c.primary_rays(rt.Params(**PT))))
    assert (ids == 0).sum() > 60 and not ke[ids == 0].any()                  # still emitters (the paths end there), adding nothing
    # ... and one lit texel brings the list back by a map-only commit
    one = np.zeros((4, 4, 4), np.uint8); one[1, 2, :3] = 200
    c.set_texture(0, one, False); c.commit()
    lit = frame(rt, c)
    assert c.lights()[:, 11].sum() > 0.99 and rays_of(c.stats())[2] > stats[0][2] and not np.array_equal(bits(lit), bits(imgs[0]))
    c.close()


# ------------------------------------------------------------------------------------------------
# 6: a tiny scene
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tiny_scene_crosses_to_the_general_path_and_back(rt, grid_world):
    cb = rt.Scene.cornell()
    cv, ci, cm = cb.meshes[0]
    mats = np.concatenate([np.asarray(cb.materials, np.float32), np.asarray(cb.materials, np.float32)[4:5]])      # one more emitting material that no triangle uses
    unused, used, light = len(mats) - 1, 1, 4
    assert unused not in set(np.asarray(cm).tolist()) and used in set(np.asarray(cm).tolist()) and mats[light, 8:11].max() > 0 and not mats[used, 8:11].any()
    plain = ArrayScene(mats, [(cv, ci, cm)], cb.instances, cb.view_proj, -1.0, 1.0)
    c = context(rt, [], plain)
    ref = frame(rt, c)
    refs = c.lights()
    fused = lambda: c.stats().kernel_launches[rt.K_BOUNCE] > 0 and c.stats().kernel_launches[rt.K_SHADE] == 0
    assert fused()
    c.set_mesh_uvs(0, np.random.default_rng(3).uniform(-1, 2, (len(ci), 2)).astype(np.float32)); c.set_texture(0, grid_world.textures[1][0], False)
    for m in (used, unused):                                                 # a map on a non-emitter or on an emitter no triangle uses never leaves the fused path
        c.set_material_map(m, 0, rt.MAP_KE); c.commit()
        img = frame(rt, c)
        assert fused() and np.array_equal(bits(img), bits(ref)) and np.array_equal(bits(c.lights()), bits(refs)), m
    c.set_material_map(light, 0, rt.MAP_KE); c.commit()
    assert c.stats().bvh_refits == 0                                         # the commit that crosses the line is a rebuild
    img = frame(rt, c)
    assert general_path(rt, c.stats()) and not np.array_equal(bits(img), bits(ref)) and img[..., :3].sum() > 0
    assert (c.emission(c.trace_closest(c.primary_rays(rt.Params(**PT))))[1] == 0).any()
    c.set_material_map(light, None, rt.MAP_KE); c.commit()
    img = frame(rt, c)
    assert fused() and np.array_equal(bits(img), bits(ref)) and np.array_equal(bits(c.lights()), bits(refs))
    c.close()


# ------------------------------------------------------------------------------------------------
# 7: the host layer's binding (BindSceneMaps) through the command line
# ------------------------------------------------------------------------------------------------
SIGN_OBJ = """mtllib sign.mtl
v -2 0 -2
v 2 0 -2
v 2 0 2
v -2 0 2
v -1 1.5 -1
v 1 1.5 -1
v 1 1.5 1
v -1 1.5 1
vt 0 0
vt 1 0
vt 1 1
vt 0 1
vn 0 1 0
vn 0 -1 0
usemtl floor
f 1/1/1 3/3/1 2/2/1
f 1/1/1 4/4/1 3/3/1
usemtl sign
f 5/1/2 6/2/2 7/3/2
f 5/1/2 7/3/2 8/4/2
"""


@pytest.mark.gpu
def test_cli_and_from_obj_render_the_same_bits(rt, tmp_path):
    """rtx_render on an OBJ whose MTL names a PPM as map_Ke binds the slot through the C++ BindSceneMaps: its image equals the Python path's (Scene.from_obj, Context.upload)
    bit for bit and differs from --no-emission-maps, which gives the image of the scene loaded with emission_maps=False (and so does --no-textures)"""
    from test_denoise import read_exr_rgb
    rng = np.random.default_rng(8)
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8); rgb[2:4] = 0
    (tmp_path / "glow.ppm").write_bytes(b"P6 7 6 255\n" + rgb.tobytes())
    (tmp_path / "sign.obj").write_text(SIGN_OBJ)
    (tmp_path / "sign.mtl").write_text("newmtl floor\nKd 0.7 0.7 0.7\nPr 0.8\n\nnewmtl sign\nKd 0.5 0.5 0.5\nKe 9 8 7\nmap_Ke glow.ppm\n")
    files, mtl = [str(tmp_path / "sign.obj")], str(tmp_path) + "/"
    exe = os.path.join(ROOT, "royaltracer-dx_amd", "rtx_render")
    w, h = 64, 48
    p = rt.Params(width=w, height=h, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0)

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run([exe, "--obj", files[0], "--mtl", str(tmp_path), "--w", str(w), "--h", str(h), "--spp", "4", "--gpus", "1", "--out", out] + list(extra),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out)

    def python(scene):
        c = rt.Context(0)
        c.upload(scene, w / h); c.clear(w, h); c.render(p)
        a = c.read_accum(); c.close()
        return a[..., :3] / np.maximum(a[..., 3:], np.float32(1.0))

    sc = rt.Scene.from_obj(files, mtl)
    assert sum(t >= 0 for t in sc.ke_maps) == 1 and sc.textures[max(sc.ke_maps)] == "glow.ppm"
    mapped = python(sc)
    plain = python(rt.Scene.from_obj(files, mtl, emission_maps=False))
    assert mapped.sum() > 0 and not np.array_equal(bits(mapped), bits(plain))
    assert np.array_equal(bits(cli("m.exr")), bits(mapped))
    assert np.array_equal(bits(cli("p.exr", "--no-emission-maps")), bits(plain))
    assert np.array_equal(bits(cli("t.exr", "--no-textures")), bits(plain))

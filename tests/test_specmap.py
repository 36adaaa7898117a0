"""Specular, roughness and metalness maps on the device (include/rtx.h: SPECULAR MAPS): the two probes against the numpy twin (tests/specmap_ref.py) bit for bit; consequence
(a) — a scene whose mapped triangles each see one texel value against the unmapped scene that carries one material per value — as whole frames, bit for bit and with equal
ray counts, over the configurations that reach another kernel; consequence (b) and the Lambert-only frame; the tiny-scene line; the commit rules; and that the map matters.
Frames are 100 x 50 (ragged against the 8 x 8 blocks), 4 spp, 3 bounces, GGX; the worlds have about 50 and 100 triangles, so that every test takes a few seconds."""
import ctypes

import numpy as np
import pytest

import normalmap_ref as nr
import specmap_ref as sr
import texture_ref as tr
from test_deform import ArrayScene, bits, random_rays

W, H = 100, 50
PT = dict(width=W, height=H, spp=4, max_bounces=3, nee_samples=1, rr_start=2)
MISS = np.uint32(0xFFFFFFFF)
ERR_INVALID, ERR_STATE = -1, -4
F = np.float32


class SpecScene(ArrayScene):
    """ArrayScene + the texture attributes Context.upload binds"""
    def __init__(self, base, uvs, textures, ks=None, pr=None, pm=None, ess_table=None, normal_maps=None, environment=None, materials=None, meshes=None):
        super().__init__(base.materials if materials is None else materials, base.meshes if meshes is None else meshes, base.instances, base._vp, base.lo, base.hi)
        self.uvs, self.textures, self.ks_maps, self.pr_maps, self.pm_maps, self.ess_table, self.normal_maps = uvs, textures, ks, pr, pm, ess_table, normal_maps
        if environment is not None:
            self.environment = environment


def camera(rt, eye, center, up, fovy_deg):
    return lambda aspect: (rt.lookat(eye, center, up), rt.perspective_fov_rh(np.radians(fovy_deg), aspect, 0.1, 100.0))


def material(rt, kd, ks, pr, pm, ke=(0, 0, 0), alpha=1.0, ni=1.0):
    m = np.zeros(32, np.float32)
    m[0:3] = kd; m[3] = alpha; m[4:7] = ks; m[7] = ni; m[8:11] = ke; m[12] = pr; m[13] = pm
    m[16:32] = rt.generate_ess_lut(float(F(pr)))
    return m


def grid(origin, du, dv, nu, nv, normal, mats, uv_of_quad):
    """an nu x nv grid of quads spanning origin + [0, 1] du + [0, 1] dv -> vertices (n, 7) (w = 0: join() sets it), indices, material per index entry, corner UVs; uv_of_quad(q,
    a, b): the UV of quad q's corner at grid coordinates (a, b) in [0, 1]^2 OF THE QUAD"""
    o, du, dv = (np.asarray(x, np.float64) for x in (origin, du, dv))
    v, idx, mid, uv = [], [], [], []
    for j in range(nv + 1):
        for i in range(nu + 1):
            v.append(list(o + du * (i / nu) + dv * (j / nv)) + list(normal) + [0.0])
    for j in range(nv):
        for i in range(nu):
            q = j * nu + i
            c = {(0, 0): j * (nu + 1) + i, (1, 0): j * (nu + 1) + i + 1, (1, 1): (j + 1) * (nu + 1) + i + 1, (0, 1): (j + 1) * (nu + 1) + i}
            for tri in (((0, 0), (1, 0), (1, 1)), ((0, 0), (1, 1), (0, 1))):
                idx += [c[k] for k in tri]
                mid += [mats[q]] * 3
                uv += [uv_of_quad(q, a, b) for a, b in tri]
    return np.array(v, np.float32), np.array(idx, np.uint32), np.array(mid, np.uint32), np.array(uv, np.float32)


def join(parts):
    v, idx, mid, uv, off = [], [], [], [], 0
    for pv, pi, pm, pu in parts:
        v.append(pv); idx.append(pi + np.uint32(off)); mid.append(pm); uv.append(pu); off += len(pv)
    return np.concatenate(v), np.concatenate(idx), np.concatenate(mid), np.concatenate(uv)


def tri_tables(meshes, uvs, instances):
    """per GLOBAL triangle id (instances in order, a mesh's triangles in order): the material (the id of its first index entry) and the corner UVs (n, 3, 2)"""
    mat, uv = [], []
    for mesh, _ in instances:
        mat.append(np.asarray(meshes[mesh][2], np.int64)[::3]); uv.append(np.asarray(uvs[mesh], np.float32).reshape(-1, 3, 2))
    return np.concatenate(mat), np.concatenate(uv)


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


# ------------------------------------------------------------------------------------------------
# 1: the probes against the twin, bit for bit
# ------------------------------------------------------------------------------------------------
P_KS_SRGB, P_ORM, P_ALL, P_KS_LIN, P_LAMP, P_NONE = range(6)      # materials: Ks through a 1 x 1 sRGB texture; one 5 x 3 file as PR and PM; one 64 x 16 texture in all three slots; Ks through
                                                                  # a linear 5 x 3, PR and PM through two other textures; the emitter (maps bound: no effect); no map


class ProbeWorld:
    """a 4 x 3 x 4 room of 2 x 2 quads per face and a lamp: 50 triangles, UVs from -0.7 to 1.8"""
    def __init__(self, rt):
        rng = np.random.default_rng(20261022)
        self.materials = np.stack([material(rt, (0.7, 0.6, 0.5), (0.9, 0.7, 0.5), 0.6, 0.3), material(rt, (0.3, 0.6, 0.7), (0.5, 0.5, 0.5), 0.9, 0.8),
                                   material(rt, (0.6, 0.7, 0.3), (1.0, 0.8, 0.6), 1.0, 1.0), material(rt, (0.8, 0.8, 0.8), (0.3, 0.6, 0.9), 0.4, 0.1),
                                   material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(12, 12, 10)), material(rt, (0.5, 0.5, 0.5), (0.2, 0.2, 0.2), 0.7, 0.0)])
        faces = [((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0)), ((-2, 3, -2), (0, 0, 4), (4, 0, 0), (0, -1, 0)), ((-2, 0, -2), (0, 3, 0), (4, 0, 0), (0, 0, 1)),
                 ((-2, 0, 2), (4, 0, 0), (0, 3, 0), (0, 0, -1)), ((-2, 0, -2), (0, 0, 4), (0, 3, 0), (1, 0, 0)), ((2, 0, -2), (0, 3, 0), (0, 0, 4), (-1, 0, 0))]
        wide = lambda q, a, b: [(q % 2 + a) / 2 * 2.5 - 0.7, (q // 2 + b) / 2 * 2.5 - 0.7]
        parts = [grid(o, dv, du, 2, 2, n, [(P_KS_SRGB, P_ORM, P_ALL, P_KS_LIN, P_NONE)[(f + q) % 5] for q in range(4)], wide) for f, (o, du, dv, n) in enumerate(faces)]
        parts.append(grid((-0.7, 2.9, -0.7), (1.4, 0, 0), (0, 0, 1.4), 1, 1, (0, -1, 0), [P_LAMP], wide))
        v, i, m, uv = join(parts)
        self.meshes, self.uvs = [(v, i, m)], [uv]
        self.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
        self.plain = ArrayScene(self.materials, self.meshes, self.instances, camera(rt, (0.0, 1.5, 1.9), (0.0, 1.3, -1.0), (0, 1, 0), 70.0), -1.9, 1.9)
        px = lambda h, w: rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        self.textures = [(px(1, 1), True), (px(5, 3), False), (px(16, 64), True), (px(5, 3), False)]
        self.ks = [0, -1, 2, 3, 2, -1]; self.pr = [-1, 1, 2, 1, 2, -1]; self.pm = [-1, 1, 2, 2, 2, -1]      # (P_ORM, P_ALL: one texture as PR and PM, its taps fetched once; P_KS_LIN: two)
        self.mapped = SpecScene(self.plain, self.uvs, self.textures, self.ks, self.pr, self.pm)
        self.unmapped = SpecScene(self.plain, self.uvs, self.textures)
        self.emits = nr.emits_device(self.materials, rt.half_round)
        self.tri_mat, self.tri_uv = tri_tables(self.meshes, self.uvs, self.instances)


@pytest.fixture(scope="module")
def probe_world(rt):
    return ProbeWorld(rt)


@pytest.mark.gpu
def test_specular_probe_equals_the_twin(rt, probe_world):
    w = probe_world
    c = context(rt, [], w.mapped)
    assert c.stats().triangles == 50 == len(w.tri_mat)
    rays = np.concatenate([c.primary_rays(rt.Params(**PT))[::2], random_rays(2000, 7, w.plain.lo, w.plain.hi)])
    rays[:, 1] = np.clip(rays[:, 1], 0.1, 2.8)                               # (origins inside the room)
    rays[-20:, 0:3] = (50.0, 50.0, 50.0); rays[-20:, 4:7] = (0.0, 1.0, 0.0)   # ... and a few that miss
    hits = c.trace_closest(rays)
    want_v, want_t = sr.specular_probe(rt.half_round, w.textures, (w.ks, w.pr, w.pm), w.materials, w.emits, w.tri_mat, w.tri_uv, hits)
    got_v, got_t = c.specular(hits)
    assert len(rays) >= 4000 and np.array_equal(bits(got_v), bits(want_v)) and np.array_equal(got_t, want_t)
    prim = hits[:, 3].copy().view(np.uint32); hit = prim != MISS
    mat = w.tri_mat[np.where(hit, prim, 0)]
    ks_t, pr_t, pm_t = sr.table_values(rt.half_round, w.materials)
    table = np.concatenate([ks_t[mat], pr_t[mat, None], pm_t[mat, None]], axis=1)
    changed = hit[:, None] & (bits(got_v) != bits(table))
    for m in range(6):
        assert (hit & (mat == m)).sum() > 50, m
    s, t = tr.interp_uv(w.tri_uv[np.where(hit, prim, 0)], hits[:, 1], hits[:, 2])
    assert (s[hit] < 0).any() and (s[hit] > 1).any() and (t[hit] < 0).any() and (t[hit] > 1).any()          # the wrap is exercised
    sel = hit & (mat == P_KS_SRGB); assert changed[sel][:, :3].any() and not changed[sel][:, 3:].any() and (got_t[sel] == [0, MISS, MISS]).all()
    sel = hit & (mat == P_ORM); assert changed[sel][:, 3].any() and changed[sel][:, 4].any() and not changed[sel][:, :3].any() and (got_t[sel] == [MISS, 1, 1]).all()
    sel = hit & (mat == P_ALL); assert changed[sel].any(axis=0).all() and (got_t[sel] == [2, 2, 2]).all()
    sel = hit & (mat == P_KS_LIN); assert changed[sel].any(axis=0).all() and (got_t[sel] == [3, 1, 2]).all()
    for m in (P_LAMP, P_NONE):                                               # an emitter's maps have no effect; a material without one keeps the table's values
        sel = hit & (mat == m); assert not changed[sel].any() and (got_t[sel] == MISS).all()
    assert (~hit).sum() >= 20 and not got_v[~hit].any() and (got_t[~hit] == MISS).all()
    c.close()
    c = context(rt, [], w.unmapped)                                          # no specular map active: the table's values, no texture
    got_v, got_t = c.specular(hits)
    assert np.array_equal(bits(got_v[hit]), bits(table[hit])) and (got_t == MISS).all() and not got_v[~hit].any()
    c.close()


@pytest.mark.gpu
def test_ess_probe_equals_the_twin(rt, probe_world):
    w = probe_world
    rng = np.random.default_rng(11)
    pr1 = np.concatenate([[0.0, 1.0, 1.5, 3.0, 0.5, 1.0 / 16.0], tr.half_round_array(rt.half_round, rng.uniform(0, 1, 40).astype(np.float32))]).astype(np.float32)
    nv1 = np.concatenate([[-0.5, 0.0, 1.0, 1.5, 1.0 / 15.0], rng.uniform(0, 1, 40)]).astype(np.float32)
    pr, nv = (x.ravel() for x in np.meshgrid(pr1, nv1))
    c = context(rt, [], w.mapped)
    lut = lambda m: w.materials[m, 16:32]
    for m in range(6):                                                       # no table set: every material's own LUT, whatever Pr' says
        assert np.array_equal(bits(c.ess(m, pr, nv)), bits(sr.ess_lut(lut(m), nv))), m
    for rows in (2, 17):
        A = rng.uniform(0.05, 1.0, (rows, 16)).astype(np.float32)
        c.set_ess_table(A); c.commit()
        for m in (P_ORM, P_ALL, P_KS_LIN):                                         # a roughness map and a table: the table, rows first
            assert np.array_equal(bits(c.ess(m, pr, nv)), bits(sr.ess_table(A, pr, nv))), (rows, m)
        for m in (P_KS_SRGB, P_NONE):                                        # no roughness map: m.LUT
            assert np.array_equal(bits(c.ess(m, pr, nv)), bits(sr.ess_lut(lut(m), nv))), (rows, m)
    c.set_ess_table(None); c.commit()
    assert np.array_equal(bits(c.ess(P_ORM, pr, nv)), bits(sr.ess_lut(lut(P_ORM), nv)))
    assert rt.lib.rtx_debug_ess(c._h, 6, None, None, 0, None) == ERR_INVALID
    c.close()
    c = context(rt, [], SpecScene(w.plain, w.uvs, w.textures, ess_table=rng.uniform(0.05, 1.0, (17, 16)).astype(np.float32)))      # a table and no map: m.LUT
    assert np.array_equal(bits(c.ess(P_ORM, pr, nv)), bits(sr.ess_lut(lut(P_ORM), nv)))
    c.close()


# ------------------------------------------------------------------------------------------------
# 2: consequence (a) — whole frames, bit for bit
# ------------------------------------------------------------------------------------------------
NB, BLK = 3, 4                                                            # the block textures: NB x NB blocks of BLK x BLK texels, one value per block
B_FLOOR_A, B_FLOOR_B, B_WALL, B_LAMP, B_PANE = range(5)                   # base materials


def block_texture(rng):
    vals = rng.integers(0, 256, (NB, NB, 4), dtype=np.uint8)
    return np.repeat(np.repeat(vals, BLK, axis=0), BLK, axis=1)


def block_uv(q, a, b):
    """quad q lies inside the interior of block (q % NB, (q // NB) % NB): texel columns [4 i + 1, 4 i + 3] of 12, where all four taps of Sample read the block's value"""
    i, j = q % NB, (q // NB) % NB
    n = NB * BLK
    return [(BLK * i + 1 + 2 * a) / n, 1.0 - (BLK * j + 3 - 2 * b) / n]


class BlockWorld:
    """a floor of 6 x 6 quads, three walls of 2 x 2, a lamp and one pane with dissolve < 1: 100 triangles, so that both sides run the general path"""
    def __init__(self, rt):
        rng = np.random.default_rng(20261023)
        self.rt = rt
        self.materials = np.stack([material(rt, (0.6, 0.55, 0.5), (0.9, 0.8, 0.7), 0.8, 0.6), material(rt, (0.4, 0.5, 0.6), (0.5, 0.5, 0.5), 1.0, 0.3),
                                   material(rt, (0.7, 0.7, 0.7), (0.3, 0.3, 0.3), 0.5, 0.2), material(rt, (0.8, 0.8, 0.8), (0.5, 0.5, 0.5), 0.5, 0.5, ke=(14, 13, 11)),
                                   material(rt, (0.5, 0.7, 0.6), (0.6, 0.6, 0.6), 0.45, 0.1, alpha=0.4, ni=1.5)])
        floor = grid((-2, 0, -2), (4, 0, 0), (0, 0, 4), 6, 6, (0, 1, 0), [(B_FLOOR_A, B_FLOOR_B)[(q + q // 6) % 2] for q in range(36)], block_uv)
        walls = [grid(o, dv, du, 2, 2, n, [B_WALL, B_FLOOR_A, B_FLOOR_B, B_WALL], block_uv) for o, du, dv, n in
                 (((-2, 0, -2), (0, 3, 0), (4, 0, 0), (0, 0, 1)), ((-2, 0, -2), (0, 0, 4), (0, 3, 0), (1, 0, 0)), ((2, 0, -2), (0, 3, 0), (0, 0, 4), (-1, 0, 0)))]
        lamp = grid((-0.6, 2.9, -1.9), (1.2, 0, 0), (0, 0, 1.0), 1, 1, (0, -1, 0), [B_LAMP], block_uv)      # (towards the back wall: the camera sees it)
        pane = grid((-1.2, 0.2, -0.3), (1.6, 0, 0.5), (0, 1.5, 0), 1, 1, (0, 0, 1), [B_PANE], lambda q, a, b: block_uv(4, a, b))
        v, i, m, uv = join([floor] + walls + [lamp, pane])
        self.floor_tris = 72
        self.meshes, self.uvs = [(v, i, m)], [uv]
        self.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
        self.plain = ArrayScene(self.materials, self.meshes, self.instances, camera(rt, (0.0, 1.6, 2.4), (0.0, 0.9, -1.0), (0, 1, 0), 65.0), -1.9, 1.9)
        # textures 0, 1: the block textures (0 sRGB: only the Ks slot honours it); 2: a normal map with relief
        nrm = rng.integers(96, 160, (6, 5, 4), dtype=np.uint8); nrm[..., 2] = 230
        self.textures = [(block_texture(rng), True), (block_texture(rng), False), (nrm, False)]
        self.ks = [0, -1, -1, 1, 1]; self.pr = [0, 1, -1, 0, 0]; self.pm = [0, -1, -1, 1, 1]      # floor A: one texture in all three; floor B: roughness only; the lamp: no effect
        self.nmaps = [2, -1, 2, -1, -1]
        self.table = rt.ess_table_rows(17)
        self.tri_mat, self.tri_uv = tri_tables(self.meshes, self.uvs, self.instances)
        self.emits = nr.emits_device(self.materials, rt.half_round)

    def mapped(self, table=True, normal=False, env=None, pad=0, maps=True):
        mats = np.concatenate([self.materials, np.repeat(self.materials[2:3], pad, axis=0)]) if pad else self.materials
        lists = (self.ks, self.pr, self.pm) if maps else (None, None, None)
        return SpecScene(self.plain, self.uvs, self.textures, *lists, self.table if table else None, self.nmaps if normal else None, env, materials=mats)

    def unmapped_equivalent(self, table=True, normal=False, env=None, pad=0):
        """the scene of consequence (a): no specular map, one material per distinct (base material, Ks', Pr', Pm') a triangle sees, LUTs from the twin"""
        rt = self.rt
        uv_mid = self.tri_uv.mean(axis=1)                                    # (any point of the triangle: the taps agree over its whole area)
        hits = np.zeros((len(self.tri_mat), 4), np.float32); hits[:, 1] = hits[:, 2] = F(1.0) / F(3.0); hits[:, 3] = np.arange(len(hits), dtype=np.uint32).view(np.float32)
        val, ids = sr.specular_probe(rt.half_round, self.textures, (self.ks, self.pr, self.pm), self.materials, self.emits, self.tri_mat, self.tri_uv, hits)
        for tex in range(2):                                                 # the premise: every triangle's taps agree, at its corners too
            for k in range(3):
                assert tr.taps_agree(self.textures[tex][0], self.tri_uv[:, k, 0], self.tri_uv[:, k, 1]).all() and tr.taps_agree(self.textures[tex][0], uv_mid[:, 0], uv_mid[:, 1]).all()
        keys, mats, tri_new = {}, [], np.zeros(len(self.tri_mat), np.uint32)
        for t, base in enumerate(self.tri_mat):
            key = (int(base),) + tuple(bits(val[t]).tolist())
            if key not in keys:
                m = self.materials[base].copy()
                m[4:7] = val[t, :3]; m[12] = val[t, 3]; m[13] = val[t, 4]
                if table and ids[t, 1] != MISS:
                    m[16:32] = sr.blend_row(self.table, val[t, 3])
                keys[key] = len(mats); mats.append((m, int(base)))
            tri_new[t] = keys[key]
        v, i, _ = self.meshes[0]
        recs = np.stack([m for m, _ in mats] + [self.materials[2]] * pad)
        nmaps = [self.nmaps[b] for _, b in mats] if normal else None
        return SpecScene(self.plain, self.uvs, self.textures, None, None, None, None, nmaps, env, materials=recs, meshes=[(v, i, np.repeat(tri_new, 3))]), len(mats)


@pytest.fixture(scope="module")
def block_world(rt):
    return BlockWorld(rt)


A_CONFIGS = ["table", "no_table", "env", "normal", "env_normal", "transmission", "compact_off", "adaptive", "mats_over_lds"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", A_CONFIGS)
def test_constant_blocks_are_the_unmapped_scene_with_more_materials(rt, block_world, config):
    w = block_world
    table = config != "no_table"
    normal = config in ("normal", "env_normal")
    env = np.random.default_rng(4).uniform(0.0, 1.5, (8, 8, 3)).astype(np.float32) if config in ("env", "env_normal") else None
    # k_shade stages the material table in LDS while lights + 160 B per material fit in 24 KB: 5 resp. ~25 materials do, 5 + 200 and ~25 + 200 do not
    pad = 200 if config == "mats_over_lds" else 0
    a = w.mapped(table, normal, env, pad)
    b, nderived = w.unmapped_equivalent(table, normal, env, pad)
    assert 15 <= nderived <= 60 and (len(b.materials) * 160 > 24576) == (pad != 0) and (len(a.materials) * 160 > 24576) == (pad != 0)
    opts = [("OPT_COMPACT_STATE", 0)] if config == "compact_off" else []
    imgs, stats = [], []
    for sc in (a, b):
        c = context(rt, opts, sc)
        assert c.stats().triangles == 100
        if config == "adaptive":
            c.clear(W, H)
            res = c.render_adaptive(rt.Params(**PT), 4, 4, 12, 0.05)
            img = c.read_accum(); stats.append((res.passes, res.chunks_converged, res.chunks_at_max, res.pixel_samples))
        else:
            img = frame(rt, c, rt.FLAG_TRANSMISSION if config == "transmission" else 0)
        st = c.stats()
        stats.append(rays_of(st))
        assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] > 0      # the general path on both sides
        imgs.append(img)
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.isfinite(imgs[0]).all() and np.array_equal(bits(imgs[0]), bits(imgs[1]))
    assert stats[:len(stats) // 2] == stats[len(stats) // 2:]


# ------------------------------------------------------------------------------------------------
# 3: consequence (b), and the Lambert-only frame
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_all_255_maps_change_nothing(rt, block_world):
    w = block_world
    white = [(np.full((5, 3, 4), 255, np.uint8), False)]
    every = [0] * len(w.materials)
    imgs, stats = [], []
    for sc in (SpecScene(w.plain, w.uvs, white, every, every, every), SpecScene(w.plain, w.uvs, white)):
        c = context(rt, [], sc)
        imgs.append(frame(rt, c)); stats.append(rays_of(c.stats()))
        _, ids = c.specular(c.trace_closest(c.primary_rays(rt.Params(**PT))[::7]))
        assert (ids != MISS).any() == (sc.ks_maps is not None)               # the maps are ACTIVE on the first side: k_shade's specular-mapped form runs there
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1])) and stats[0] == stats[1]


@pytest.mark.gpu
def test_lambert_only_reads_none_of_them(rt, block_world):
    w = block_world
    imgs, stats, launches = [], [], []
    for sc in (w.mapped(table=True), w.mapped(table=False, maps=False)):
        c = context(rt, [], sc)
        imgs.append(frame(rt, c, rt.FLAG_LAMBERT_ONLY)); st = c.stats()
        stats.append(rays_of(st)); launches.append(list(st.kernel_launches))
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1])) and stats[0] == stats[1]
    assert launches[0] == launches[1] and launches[0][rt.K_SHADE] > 0


# ------------------------------------------------------------------------------------------------
# 4: a tiny scene
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tiny_scene_crosses_to_the_general_path_and_back(rt, block_world):
    cb = rt.Scene.cornell()
    cv, ci, cm = cb.meshes[0]
    mats = np.concatenate([np.asarray(cb.materials, np.float32), np.asarray(cb.materials, np.float32)[1:2]])      # one more material that no triangle uses
    unused, used, light = len(mats) - 1, 1, 4
    assert unused not in set(np.asarray(cm).tolist()) and used in set(np.asarray(cm).tolist()) and mats[light, 8:11].max() > 0 and not mats[used, 8:11].any()
    plain = ArrayScene(mats, [(cv, ci, cm)], cb.instances, cb.view_proj, -1.0, 1.0)
    c = context(rt, [], plain)
    ref = frame(rt, c)
    fused = lambda: c.stats().kernel_launches[rt.K_BOUNCE] > 0 and c.stats().kernel_launches[rt.K_SHADE] == 0
    assert fused()
    c.set_mesh_uvs(0, np.random.default_rng(3).uniform(-1, 2, (len(ci), 2)).astype(np.float32)); c.set_texture(0, block_world.textures[1][0], False)
    for m in (light, unused):                                                # a map on the emitter or on a material no triangle uses never leaves the fused path
        c.set_material_map(m, 0, rt.MAP_PR); c.commit()
        img = frame(rt, c)
        assert fused() and np.array_equal(bits(img), bits(ref)), m
    c.set_material_map(used, 0, rt.MAP_PR); c.commit()
    frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] == 0 and c.stats().kernel_launches[rt.K_SHADE] > 0
    c.set_material_map(used, None, rt.MAP_PR); c.commit()
    img = frame(rt, c)
    assert fused() and np.array_equal(bits(img), bits(ref))
    c.close()


# ------------------------------------------------------------------------------------------------
# 5: commits, state, errors
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_commit_rules_and_errors(rt, block_world, tmp_path):
    w = block_world
    L = rt.lib
    c = context(rt, [], w.mapped(table=True))
    p = rt.Params(**PT)
    ref = frame(rt, c)
    refits, tree = c.stats().bvh_refits, c.tree_hash()
    # a map-only and a table-only commit upload tables only
    c.set_material_map(B_WALL, 1, rt.MAP_PM)
    assert L.rtx_render(c._h, ctypes.byref(p)) == ERR_STATE                  # rendering before the commit
    c.commit()
    assert (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    c.set_ess_table(w.table[::2].copy())
    assert L.rtx_render(c._h, ctypes.byref(p)) == ERR_STATE
    c.commit()
    assert (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    assert not np.array_equal(bits(frame(rt, c)), bits(ref))
    c.set_material_map(B_WALL, None, rt.MAP_PM); c.set_ess_table(w.table); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(ref)) and (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)
    # rtx_save_scene_cache with a specular map bound
    assert L.rtx_save_scene_cache(c._h, str(tmp_path / "s.rtxscn").encode()) == ERR_STATE
    # invalid calls leave the committed scene untouched: the next frame's bits are equal
    bad_table = w.table.copy(); bad_table[16, 15] = np.nan
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for slot in (5, 7, 9, 11):
        assert L.rtx_set_material_map(c._h, B_WALL, slot, 0) == ERR_INVALID, slot
    assert L.rtx_set_material_map(c._h, len(w.materials), rt.MAP_PR, 0) == ERR_INVALID and L.rtx_set_material_map(c._h, B_WALL, rt.MAP_KS, len(w.textures)) == ERR_INVALID
    assert L.rtx_set_material_map(c._h, B_WALL, rt.MAP_PM, -2) == ERR_INVALID
    for rows in (1, 257):
        big = np.ones((rows, 16), np.float32)
        assert L.rtx_set_ess_table(c._h, ptr(big), rows) == ERR_INVALID, rows
    assert L.rtx_set_ess_table(c._h, ptr(bad_table), 17) == ERR_INVALID and L.rtx_set_ess_table(c._h, None, 17) == ERR_INVALID
    assert np.array_equal(bits(frame(rt, c)), bits(ref))                     # (still committed: no RTX_ERR_STATE)
    # rtx_set_materials resets the three slots and keeps the table
    rays = c.primary_rays(p)[::5]; hits = c.trace_closest(rays)
    assert (c.specular(hits)[1] != MISS).any()
    c.set_materials(w.materials); c.commit()
    assert (c.specular(hits)[1] == MISS).all()
    plain = frame(rt, c)
    assert not np.array_equal(bits(plain), bits(ref))
    c.set_material_map(B_FLOOR_B, 1, rt.MAP_PR); c.commit()
    pr = np.linspace(0, 1, 9, dtype=np.float32); nv = np.full(9, 0.6, np.float32)
    assert np.array_equal(bits(c.ess(B_FLOOR_B, pr, nv)), bits(sr.ess_table(w.table, pr, nv)))
    c.close()
    c = context(rt, [], w.mapped(table=False, maps=False))                   # the frame after rtx_set_materials was the frame of the scene without maps
    assert np.array_equal(bits(frame(rt, c)), bits(plain))
    c.close()


# ------------------------------------------------------------------------------------------------
# 6: the maps matter
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_roughness_map_changes_its_triangles_only(rt, block_world):
    """floor B's only map is its roughness map, whose blocks hold different values: against the unmapped frame the pixels that see floor B first change (8 spp: most of them —
    more than half is asked for), the pixels that see the lamp first do not (an emitter is not shaded: its radiance is Ke, to the bit)"""
    w = block_world
    none = [-1] * len(w.materials)
    only_b = [1 if m == B_FLOOR_B else -1 for m in range(len(w.materials))]
    px = w.textures[1][0]
    assert len(np.unique(px[::BLK, ::BLK, 1])) >= 2
    imgs = []
    for pr in (only_b, none):
        c = context(rt, [], SpecScene(w.plain, w.uvs, w.textures, none, pr, none, w.table))
        imgs.append(frame(rt, c, spp=8))
        if pr is only_b:
            prim = c.trace_closest(c.primary_rays(rt.Params(**PT)))[:, 3].copy().view(np.uint32).reshape(H, W)
        c.close()
    mat = np.where(prim != MISS, w.tri_mat[np.where(prim != MISS, prim, 0)], -1)
    diff = (bits(imgs[0]) != bits(imgs[1])).any(axis=-1)
    on_b, on_lamp = mat == B_FLOOR_B, mat == B_LAMP
    assert on_b.sum() > 300 and on_lamp.sum() > 20
    assert diff[on_b].mean() > 0.5 and not diff[on_lamp].any()


# ------------------------------------------------------------------------------------------------
# 7: the host layer's binding (BindSceneMaps) through the command line
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_binds_the_maps_and_the_table(rt, tmp_path):
    """rtx_render on an OBJ whose MTL names map_Ks / map_Pr / map_Pm images binds the three slots and a 17-row table through the C++ BindSceneMaps: its image equals the
    Python path's (Context.upload: the same lists, ess_table_rows(17)) bit for bit, differs from --no-spec-maps, and --no-spec-maps / --no-textures give the image of the
    scene loaded with spec_maps=False; the table matters (the Python path without it gives another image), so the CLI's table is the 17 rows"""
    import os
    import subprocess
    from test_cutout_ref import write_card
    from test_denoise import read_exr_rgb
    rng = np.random.default_rng(8)
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    (tmp_path / "orm.ppm").write_bytes(b"P6 7 6 255\n" + rgb.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
    w, h = 64, 48
    p = rt.Params(width=w, height=h, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0)

    def cli(files, name, *extra):
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

    files, mtl = write_card(tmp_path, "map_Ks orm.ppm\nmap_Pr orm.ppm\nmap_Pm orm.ppm\n")
    sc = rt.Scene.from_obj(files, mtl)
    assert sc.ks_maps == sc.pr_maps == sc.pm_maps == [-1, -1, 0, -1] and sc.ess_table is not None
    mapped = python(sc)
    sc.ess_table = None
    no_table = python(sc)
    plain = python(rt.Scene.from_obj(files, mtl, spec_maps=False))
    assert mapped.sum() > 0 and not np.array_equal(bits(mapped), bits(plain)) and not np.array_equal(bits(mapped), bits(no_table))
    assert np.array_equal(bits(cli(files, "m.exr")), bits(mapped))
    assert np.array_equal(bits(cli(files, "p.exr", "--no-spec-maps")), bits(plain))
    assert np.array_equal(bits(cli(files, "t.exr", "--no-textures")), bits(plain))
    # a metalness map alone: bound, no roughness map, so no table is set — the image of the Python path with the list and without a table
    files, mtl = write_card(tmp_path, "Ks 0.6 0.6 0.6\nPr 0.4\nmap_Pm orm.ppm\n")
    sc = rt.Scene.from_obj(files, mtl)
    assert sc.pm_maps == [-1, -1, 0, -1] and sc.pr_maps == [-1] * 4 and sc.ess_table is None
    only_pm = python(sc)
    assert np.array_equal(bits(cli(files, "q.exr")), bits(only_pm)) and not np.array_equal(bits(only_pm), bits(python(rt.Scene.from_obj(files, mtl, spec_maps=False))))

"""Tangent-space normal maps on the device (include/rtx.h: NORMAL MAPS): the tangent table and the shading-normal probe against the numpy twin (tests/normalmap_ref.py) bit
for bit; a scene whose normal maps hold only flat texels against the scene with none bound, bit for bit, over the configurations that reach another kernel or commit path;
the direction of the effect on a floor lit from one side; and the plumbing (the emitter's map, the passes that ignore maps, errors and state, the command line) against itself.
The world is small — about 200 triangles, frames of 64 x 48 — so that every test takes a few seconds."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import normalmap_ref as nr
from test_deform import ArrayScene, bits, place, random_rays

W, H = 64, 48
PT = dict(width=W, height=H, spp=4, max_bounces=4, nee_samples=1, rr_start=2)
ROOM, PANEL = 0, 1                                   # meshes
M_A, M_B, M_FLAT, M_LAMP, M_ALL, M_NONE = range(6)   # materials: 8 x 8 map, 5 x 3 map, flat map, the emitter (a map bound: no effect), map_Kd + cut-out + normal map, no map
NMAP = {M_A: 0, M_B: 1, M_FLAT: 2, M_LAMP: 0, M_ALL: 1}
MISS = np.uint32(0xFFFFFFFF)
ERR_STATE = -4                                       # RTX_ERR_STATE


class NrmScene(ArrayScene):
    """ArrayScene + the texture attributes Context.upload binds"""
    def __init__(self, base, uvs, textures, normal_maps, material_maps=None, opacity_maps=None, environment=None):
        super().__init__(base.materials, base.meshes, base.instances, base._vp, base.lo, base.hi)
        self.uvs, self.textures, self.normal_maps, self.material_maps, self.opacity_maps = uvs, textures, normal_maps, material_maps, opacity_maps
        if environment is not None:
            self.environment = environment


def camera(rt, eye, center, up, fovy_deg):
    return lambda aspect: (rt.lookat(eye, center, up), rt.perspective_fov_rh(np.radians(fovy_deg), aspect, 0.1, 100.0))


def grid(origin, du, dv, nu, nv, normal, base, mats):
    """an nu x nv grid of quads spanning origin + [0, 1] du + [0, 1] dv: vertices (n, 7), indices, material id per index entry (mats: per quad), corner UVs = (a, b) of the span"""
    o, du, dv = (np.asarray(x, np.float64) for x in (origin, du, dv))
    v, idx, mid, uv = [], [], [], []
    for j in range(nv + 1):
        for i in range(nu + 1):
            v.append(list(o + du * (i / nu) + dv * (j / nv)) + list(normal) + [float(base)])
    for j in range(nv):
        for i in range(nu):
            q = j * (nu + 1) + i
            for tri in ((q, q + 1, q + nu + 2), (q, q + nu + 2, q + nu + 1)):
                idx += tri
                mid += [mats[j * nu + i]] * 3
                uv += [[(k % (nu + 1)) / nu, (k // (nu + 1)) / nv] for k in tri]
    return np.array(v, np.float32), np.array(idx, np.uint32), np.array(mid, np.uint32), np.array(uv, np.float32)


def join(parts, base):
    v, idx, mid, uv, off = [], [], [], [], 0
    for pv, pi, pm, pu in parts:
        pv = pv.copy(); pv[:, 6] = float(base)
        v.append(pv); idx.append(pi + np.uint32(off)); mid.append(pm); uv.append(pu); off += len(pv)
    return np.concatenate(v), np.concatenate(idx), np.concatenate(mid), np.concatenate(uv)


class World:
    def __init__(self, rt):
        rng = np.random.default_rng(20261021)
        cb = np.asarray(rt.Scene.cornell().materials, np.float32)
        grey, lamp = cb[1], cb[4]
        mats = np.stack([grey, grey, grey, lamp, grey, grey]).copy()
        for m, kd in ((M_A, (0.7, 0.6, 0.5)), (M_B, (0.3, 0.6, 0.7)), (M_FLAT, (0.6, 0.7, 0.3)), (M_ALL, (0.8, 0.8, 0.8)), (M_NONE, (0.5, 0.5, 0.5))):
            mats[m, :3] = kd
        # the room: six faces of a 4 x 3 x 4 box seen from inside, 3 x 3 quads each (108 triangles), and a lamp under the ceiling (2)
        # (origin, dv, du, inward normal = du x dv)
        faces = [((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0)), ((-2, 3, -2), (0, 0, 4), (4, 0, 0), (0, -1, 0)), ((-2, 0, -2), (0, 3, 0), (4, 0, 0), (0, 0, 1)),
                 ((-2, 0, 2), (4, 0, 0), (0, 3, 0), (0, 0, -1)), ((-2, 0, -2), (0, 0, 4), (0, 3, 0), (1, 0, 0)), ((2, 0, -2), (0, 3, 0), (0, 0, 4), (-1, 0, 0))]
        parts = [grid(o, dv, du, 3, 3, n, 0, [(M_A, M_B, M_FLAT, M_NONE, M_ALL)[(f + q) % 5] for q in range(9)]) for f, (o, du, dv, n) in enumerate(faces)]
        parts.append(grid((-0.5, 2.9, -0.5), (1, 0, 0), (0, 0, 1), 1, 1, (0, -1, 0), 0, [M_LAMP]))
        room = join(parts, 0)
        # the panel: a 5 x 4 grid (40 triangles) with a bumpy surface, smooth normals that are not the face normals, UVs beyond [0, 1]; one row of quads has collinear UVs
        # (a zero tangent record under a non-flat map) and one row has UVs mirrored along u
        pv, pi, pm, pu = grid((-0.5, -0.4, 0), (1, 0, 0), (0, 0.8, 0), 5, 4, (0, 0, 1), len(room[2]), [(M_A, M_B, M_ALL, M_FLAT, M_A)[q % 5] for q in range(20)])
        pv[:, 2] = rng.uniform(-0.05, 0.05, len(pv)); nrm = pv[:, 3:6] + rng.uniform(-0.2, 0.2, (len(pv), 3)); pv[:, 3:6] = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        pu = pu * np.float32(2.5) - np.float32(0.7)
        pu3 = pu.reshape(-1, 3, 2)
        pu3[0:10, :, 1] = pu3[0:10, :, 0]                              # row 0: v = u at every corner -> det = 0
        pu3[10:20, :, 0] = np.float32(1.0) - pu3[10:20, :, 0]          # row 1: mirrored
        pm3 = pm.reshape(-1, 3); pm3[0:10] = M_A
        self.meshes = [(room[0], room[1], room[2]), (pv, pi, pm)]
        self.uvs = [room[3], pu]
        mirrored = np.array([[-0.9, 0.3, 0, 0], [0.2, 1.7, 0.1, 0], [0, -0.2, 1.3, 0], [0.9, 1.4, 0.6, 1]], np.float32).reshape(16)      # det < 0, non-uniform
        turned = np.array([[0.6, 0, -0.8, 0], [0, 1, 0, 0], [0.8, 0, 0.6, 0], [-0.8, 1.2, -0.3, 1]], np.float32).reshape(16)
        self.instances = [(ROOM, np.eye(4, dtype=np.float32).reshape(16)), (PANEL, turned), (PANEL, mirrored)]
        self.turned2 = place(-0.6, 1.0, -0.5, 1.2, 0.9, 1.0)
        eye, center = (0.0, 1.5, 1.9), (0.0, 1.3, -1.0)
        self.plain = ArrayScene(mats, self.meshes, self.instances, camera(rt, eye, center, (0, 1, 0), 70.0), -1.9, 1.9)
        kd = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8); kd[..., 3] = np.where(rng.uniform(size=(8, 8)) < 0.3, 0, 255)
        self.textures = [(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8), False), (rng.integers(0, 256, (3, 5, 4), dtype=np.uint8), True), (self.flat(rng, 4, 4), False), (kd, True)]
        self.flat_textures = [(self.flat(rng, 8, 8), False), (self.flat(rng, 3, 5), True), self.textures[2], self.textures[3]]
        n = len(mats)
        self.nmaps = [NMAP.get(m, -1) for m in range(n)]
        self.kd_maps = [3 if m == M_ALL else -1 for m in range(n)]
        self.none = [-1] * n
        self.mapped = NrmScene(self.plain, self.uvs, self.textures, self.nmaps, self.kd_maps, self.kd_maps)
        self.flat_mapped = NrmScene(self.plain, self.uvs, self.flat_textures, self.nmaps, self.kd_maps, self.kd_maps)
        self.unmapped = NrmScene(self.plain, self.uvs, self.textures, self.none, self.kd_maps, self.kd_maps)
        self.emits = (mats[:, 8:11] > 0).any(axis=1)
        self.rng = rng

    @staticmethod
    def flat(rng, h, w):
        px = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        px[..., 0] = 128; px[..., 1] = 128; px[..., 2] = rng.integers(129, 256, (h, w))
        return px

    def tables(self, meshes=None, instances=None):
        """per GLOBAL triangle id: corner UVs (n, 3, 2) and the twin's tangent records; per instance its matrix"""
        meshes, instances = meshes or self.meshes, instances or self.instances
        uv, tan = [], []
        for mesh, _ in instances:
            v, i, _ = meshes[mesh]
            p3 = np.asarray(v, np.float32).reshape(-1, 7)[np.asarray(i, np.int64), :3].reshape(-1, 3, 3)
            uv3 = np.asarray(self.uvs[mesh], np.float32).reshape(-1, 3, 2)
            uv.append(uv3); tan.append(nr.tangent_records(p3, uv3))
        return np.concatenate(uv), np.concatenate(tan), np.stack([np.asarray(m, np.float32) for _, m in instances])


@pytest.fixture(scope="module")
def world(rt):
    return World(rt)


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


# ------------------------------------------------------------------------------------------------
# 1, 2: the tangent table and the probe, bit for bit
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gpu_build", [0, 1])
def test_tangent_table_equals_the_twin(rt, world, gpu_build):
    c = context(rt, [("OPT_GPU_BUILD", gpu_build)], world.mapped)
    _, tan, _ = world.tables()
    assert len(tan) == c.stats().triangles == 190 and tan.any()
    assert np.array_equal(bits(c.tri_tangents()), bits(tan))
    assert np.array_equal(bits(c.tri_tangents(110, 7)), bits(tan[110:117]))
    assert not tan[110:120].any() and tan[120:130].any()                     # the collinear row of the first panel instance; its mirrored row
    # object space: a transform-only commit does not touch it
    c.set_instance_transform(1, world.turned2); c.commit()
    assert np.array_equal(bits(c.tri_tangents()), bits(tan))
    # new vertices: re-derived for that mesh (both of its instances), the other mesh's records stay
    v = np.array(world.meshes[PANEL][0], np.float32, copy=True)
    v[:, 0] *= np.float32(1.3); v[:, 2] += np.float32(0.1) * np.sin(v[:, 1] * np.float32(5.0))
    c.update_mesh_vertices(PANEL, v); c.commit()
    meshes = [world.meshes[ROOM], (v, world.meshes[PANEL][1], world.meshes[PANEL][2])]
    _, tan2, _ = world.tables(meshes)
    assert not np.array_equal(bits(tan2[110:]), bits(tan[110:])) and np.array_equal(bits(tan2[:110]), bits(tan[:110]))
    assert np.array_equal(bits(c.tri_tangents()), bits(tan2))
    c.close()
    # no normal map active: RTX_ERR_STATE
    c = context(rt, [], world.unmapped)
    assert rt.lib.rtx_debug_tri_tangents(c._h, 0, 0, None) == ERR_STATE
    c.close()


@pytest.mark.gpu
def test_shading_normal_probe_equals_the_twin(rt, world):
    c = context(rt, [], world.mapped)
    p = rt.Params(**PT)
    aimed = random_rays(1000, 8, world.plain.lo, world.plain.hi)             # ... at the two panel instances, from either side
    rng = np.random.default_rng(9)
    for k, (_, m) in enumerate(world.instances[1:]):
        M = np.asarray(m, np.float64).reshape(4, 4)
        q = np.stack([rng.uniform(-0.5, 0.5, 500), rng.uniform(-0.4, 0.4, 500), np.zeros(500)], 1) @ M[:3, :3] + M[3, :3]
        d = q - aimed[k::2, 0:3]
        aimed[k::2, 4:7] = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    rays = np.concatenate([c.primary_rays(p)[::3], random_rays(2000, 7, world.plain.lo, world.plain.hi), aimed])
    rays[:, 1] = np.clip(rays[:, 1], 0.1, 2.8)                               # (origins inside the room)
    hits = c.trace_closest(rays)
    surf = c.surface(rays, hits)
    uv3, tan, o2w = world.tables()
    br = {}
    want = nr.shading_normal_probe(world.textures, world.nmaps, world.emits, uv3, tan, surf, o2w, rays, hits, br)
    got = c.shading_normal(rays, hits)
    assert len(rays) >= 4000 and np.array_equal(bits(got), bits(want))
    prim = hits[:, 3].view(np.uint32); hit = prim != MISS
    tex = got[:, 3].view(np.uint32); mat = surf[:, 3].view(np.uint32); inst = surf[:, 8].view(np.uint32)
    changed = hit & (bits(got[:, :3]) != bits(surf[:, 4:7])).any(axis=1)
    wo = -rays[:, 4:7]
    behind = (surf[:, 4:7] * wo).sum(axis=1) < 0
    # every branch of the definition is taken, counted on the twin; enough records are left that the map changes for the sub-counts below to mean something
    assert br["guard"].any() and br["flat"].any() and br["degenerate"].any() and changed.any()
    assert (changed & behind).any() and (changed & (inst == 2)).any() and (changed & (inst == 1)).any() and (changed & (inst == 0)).any()
    print("records", len(rays), "guard", br["guard"].sum(), "flat", br["flat"].sum(), "degenerate", br["degenerate"].sum(), "changed", changed.sum(), "from behind", (changed & behind).sum(),
          "mirrored instance", (changed & (inst == 2)).sum())
    lampm = hit & (mat == M_LAMP)
    assert lampm.any() and (tex[lampm] == MISS).all() and np.array_equal(bits(got[lampm, :3]), bits(surf[lampm, 4:7]))
    nomap = hit & (mat == M_NONE)
    assert nomap.any() and (tex[nomap] == MISS).all() and not changed[nomap].any()
    assert (tex[hit & (mat == M_ALL)] == 1).all() and (tex[hit & (mat == M_FLAT)] == 2).all() and not changed[hit & (mat == M_FLAT)].any()
    if (~hit).any():
        assert not got[~hit, :3].any() and (tex[~hit] == MISS).all()
    c.close()
    # no normal map active: surface()'s normal, no texture
    c = context(rt, [], world.unmapped)
    got = c.shading_normal(rays, hits)
    assert np.array_equal(bits(got[hit, :3]), bits(surf[hit, 4:7])) and (got[:, 3].view(np.uint32) == MISS).all()
    c.close()


# ------------------------------------------------------------------------------------------------
# 3: flat maps change nothing, to the bit
# ------------------------------------------------------------------------------------------------
def tiny_scenes(rt, world):
    cb = rt.Scene.cornell()
    cv, ci, cm = cb.meshes[0]
    plain = ArrayScene(np.asarray(cb.materials, np.float32), [(cv, ci, cm)], cb.instances, cb.view_proj, -1.0, 1.0)
    uvs = [np.random.default_rng(3).uniform(-1, 2, (len(ci), 2)).astype(np.float32)]
    return plain, NrmScene(plain, uvs, world.flat_textures, [0, 1, 2, 0, 1])


FLAT_CONFIGS = ["default", "compact_off", "gpu_build", "shards", "adaptive", "transmission", "environment", "tiny"]


@pytest.mark.gpu
@pytest.mark.parametrize("config", FLAT_CONFIGS)
def test_flat_maps_are_the_unmapped_scene(rt, world, config):
    opts = {"compact_off": [("OPT_COMPACT_STATE", 0)], "gpu_build": [("OPT_GPU_BUILD", 1)]}.get(config, [])
    a, b = world.flat_mapped, world.unmapped
    if config == "environment":
        env = np.random.default_rng(4).uniform(0.0, 2.0, (8, 8, 3)).astype(np.float32)
        a = NrmScene(world.plain, world.uvs, world.flat_textures, world.nmaps, world.kd_maps, world.kd_maps, env)
        b = NrmScene(world.plain, world.uvs, world.flat_textures, world.none, world.kd_maps, world.kd_maps, env)
    if config == "tiny":
        b, a = tiny_scenes(rt, world)
    imgs, stats = [], []
    for sc, extra in ((a, []), (b, [("OPT_SMALL_SCENE", 0)] if config == "tiny" else [])):
        c = context(rt, opts + extra, sc)
        assert rt.lib.rtx_debug_tri_tangents(c._h, 0, 0, None) == (0 if sc is a else ERR_STATE)      # the flat maps are ACTIVE: k_shade's normal-mapped form runs on that side
        if config == "shards":
            c.clear(W, H)
            for r in range(2):
                c.render(rt.Params(tile_size=16, shard_rank=r, shard_count=2, **PT))
            img = c.read_accum()
        elif config == "adaptive":
            c.clear(W, H)
            res = c.render_adaptive(rt.Params(**PT), 4, 4, 12, 0.05)
            img = c.read_accum(); stats.append((res.passes, res.chunks_converged, res.chunks_at_max, res.pixel_samples))
        else:
            img = frame(rt, c, rt.FLAG_TRANSMISSION if config == "transmission" else 0)
        st = c.stats()
        stats.append((st.rays_primary, st.rays_extension, st.rays_shadow))
        if config == "tiny":
            assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] > 0      # the general path on both sides
        imgs.append(img)
        c.close()
    assert imgs[0][..., :3].sum() > 0 and np.array_equal(bits(imgs[0]), bits(imgs[1]))
    assert stats[:len(stats) // 2] == stats[len(stats) // 2:]


@pytest.mark.gpu
def test_tiny_scene_returns_to_the_fused_path(rt, world):
    """the commit that binds a normal map to a used material takes the Cornell box to the general path, the commit that unbinds it takes it back; an emitter's map does neither"""
    plain, mapped = tiny_scenes(rt, world)
    c = context(rt, [], plain)
    ref = frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] > 0
    c.set_mesh_uvs(0, mapped.uvs[0]); c.set_texture(0, world.flat_textures[0][0], False)
    c.set_material_map(4, 0, rt.MAP_NORMAL); c.commit()                       # material 4 is the light
    frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] > 0
    c.set_material_map(1, 0, rt.MAP_NORMAL); c.commit()
    frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] == 0 and c.stats().kernel_launches[rt.K_SHADE] > 0
    c.set_material_map(1, None, rt.MAP_NORMAL); c.commit()
    img = frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] > 0 and np.array_equal(bits(img), bits(ref))
    c.close()


# ------------------------------------------------------------------------------------------------
# 4: the map matters, and in the right direction
# ------------------------------------------------------------------------------------------------
def floor_scene(rt, o2w, mirror_uv, green):
    """a 2 x 2 floor quad in the plane z = 0 (normal +z, u along +x, v along +y; mirror_uv: u along -x) instanced through o2w, a small emitter at distance 6 in the
    direction 45 degrees from the floor normal towards the WORLD image of +T (green: of +B), facing the floor, and the camera straight above with a narrow field of view"""
    cb = np.asarray(rt.Scene.cornell().materials, np.float32)
    mats = np.stack([cb[1], cb[4]]).copy()
    fv, fi, fm, fu = grid((-1, -1, 0), (2, 0, 0), (0, 2, 0), 1, 1, (0, 0, 1), 0, [0])
    if mirror_uv:
        fu[:, 0] = np.float32(1.0) - fu[:, 0]
    M = np.asarray(o2w, np.float64).reshape(4, 4)
    axis = np.array([0.0, 1.0, 0.0]) if green else np.array([-1.0 if mirror_uv else 1.0, 0.0, 0.0])      # +B, or +T, in object space
    t_world = axis @ M[:3, :3]
    d = (t_world / np.linalg.norm(t_world) + np.array([0.0, 0.0, 1.0])) / np.sqrt(2.0)
    centre = 6.0 * d
    a = np.cross(d, [0.0, 0.0, 1.0]); a /= np.linalg.norm(a); b = np.cross(a, d)
    lv, li, lm, lu = grid(centre - 0.15 * a - 0.15 * b, 0.3 * a, 0.3 * b, 1, 1, -d, len(fm), [1])      # (du x dv = a x b = -d: the emitter faces the floor)
    eye = (0.0, 0.0, 8.0)
    base = ArrayScene(mats, [(fv, fi, fm), (lv, li, lm)], [(0, np.asarray(o2w, np.float32).reshape(16)), (1, np.eye(4, dtype=np.float32).reshape(16))],
                      camera(rt, eye, (0.0, 0.0, 0.0), (0, 1, 0), 10.0), -1.0, 1.0)
    return base, [fu, lu]


DIRECTION_CASES = {"red": (np.eye(4), False, False), "green": (np.eye(4), False, True), "mirrored_instance": (np.diag([-1.0, 1.0, 1.0, 1.0]), False, False),
                   "mirrored_uvs": (np.eye(4), True, False)}


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(DIRECTION_CASES))
def test_the_tilt_goes_towards_the_light(rt, case):
    """mean radiance over the floor's pixels: towards > flat > away, and away < 0.5 x flat.  Across the floor the light direction varies by at most about 10 degrees: flat sees
    cos in [0.57, 0.82], away (the normal turned 45 degrees from the light's side) sees cos <= 0.17, a ratio of at most 0.30"""
    o2w, mirror_uv, green = DIRECTION_CASES[case]
    base, uvs = floor_scene(rt, o2w, mirror_uv, green)
    texel = lambda r: np.array([[[128, r, 219, 255] if green else [r, 128, 219, 255]]], np.uint8)
    means = {}
    c = context(rt, [], NrmScene(base, uvs, [(texel(219), False), (np.array([[[128, 128, 255, 255]]], np.uint8), False), (texel(37), False)], [0, -1]))
    for name, tex in (("towards", 0), ("flat", 1), ("away", 2)):
        c.set_material_map(0, tex, rt.MAP_NORMAL); c.commit()
        img = frame(rt, c, rt.FLAG_LAMBERT_ONLY, spp=16, max_bounces=1, nee_samples=1)
        rgb = img[..., :3] / np.maximum(img[..., 3:], np.float32(1.0))
        means[name] = float(rgb.mean())
    c.close()
    print(case, means)
    assert means["towards"] > means["flat"] > means["away"] >= 0.0 and means["flat"] > 0.0, means
    assert means["away"] < 0.5 * means["flat"], means


# ------------------------------------------------------------------------------------------------
# 5, 6: the emitter's map; who ignores normal maps
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_an_emitters_map_has_no_effect(rt, world):
    only_lamp = [0 if m == M_LAMP else -1 for m in range(6)]
    c = context(rt, [], NrmScene(world.plain, world.uvs, world.textures, only_lamp, world.kd_maps, world.kd_maps))
    lights, img = c.lights(), frame(rt, c)
    assert rt.lib.rtx_debug_tri_tangents(c._h, 0, 0, None) == ERR_STATE             # not active: no triangle of a non-emitting material has a map
    c.close()
    c = context(rt, [], world.unmapped)
    assert np.array_equal(bits(c.lights()), bits(lights)) and len(lights) == 2
    assert np.array_equal(bits(frame(rt, c)), bits(img))
    c.close()


@pytest.mark.gpu
def test_the_other_passes_ignore_normal_maps(rt, world):
    out = []
    p = rt.Params(**PT)
    for sc in (world.mapped, world.unmapped):
        c = context(rt, [], sc)
        rays = c.primary_rays(p)
        hits = c.trace_closest(rays)
        got = {"surface": c.surface(rays, hits), "guides": c.denoise_guides(W, H), "layer10": c.read_layer(10, W, H)}
        c.clear(W, H); c.render_v6_pass1(p); got["pass1"] = c.read_accum()
        vp = sc.view_proj(W / H)
        c.set_camera(*vp); c.set_camera(*vp); c.restir_reset()                # previous view = current view
        c.clear(W, H); c.render_restir(rt.Params(**dict(PT, spp=2, max_bounces=3, nee_samples=4))); got["restir"] = c.read_accum()
        got["frame"] = frame(rt, c)
        out.append(got); c.close()
    for k in ("surface", "guides", "layer10", "pass1", "restir"):
        assert np.array_equal(out[0][k].view(np.uint8), out[1][k].view(np.uint8)), k
    assert not np.array_equal(bits(out[0]["frame"]), bits(out[1]["frame"]))   # ... and rtx_render does not


# ------------------------------------------------------------------------------------------------
# 7: errors and state
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_and_state(rt, world, tmp_path):
    c = context(rt, [], world.mapped)
    L, h = rt.lib, c._h
    ref = frame(rt, c)
    ntex = len(world.textures)
    for mat, slot, tex in ((6, 4, 0), (0, 4, ntex), (0, 4, -2), (0, 1, 0), (0, 3, 0), (0, 5, 0)):
        assert L.rtx_set_material_map(h, mat, slot, tex) == -1, (mat, slot, tex)
    assert np.array_equal(bits(frame(rt, c)), bits(ref))                      # refused calls leave the scene committed and untouched
    # a map-only commit on a resident scene uploads tables only
    st0, hash0 = c.stats().bvh_refits, c.tree_hash()
    c.set_material_map(M_NONE, 0, rt.MAP_NORMAL)
    with pytest.raises(rt.RtxError):
        frame(rt, c)                                                          # RTX_ERR_STATE between the call and the commit
    assert L.rtx_render(h, ctypes.byref(rt.Params(**PT))) == ERR_STATE
    c.commit()
    changed = frame(rt, c)
    assert c.stats().bvh_refits == st0 and c.tree_hash() == hash0 and not np.array_equal(bits(changed), bits(ref))
    c.set_material_map(M_NONE, None, rt.MAP_NORMAL); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(ref)) and c.stats().bvh_refits == st0 and c.tree_hash() == hash0
    # the scene cache holds no texels
    with pytest.raises(rt.RtxError):
        c.save_scene_cache(tmp_path / "a.rtxscn")
    # rtx_set_materials unbinds every slot
    c.set_materials(world.plain.materials); c.commit()
    assert L.rtx_debug_tri_tangents(h, 0, 0, None) == ERR_STATE
    plain = context(rt, [], world.plain)
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, plain)))
    plain.close()
    c.save_scene_cache(tmp_path / "b.rtxscn")
    assert os.path.getsize(tmp_path / "b.rtxscn") > 0
    c.close()


# ------------------------------------------------------------------------------------------------
# 8: the command line
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_renders_norm_and_bump(rt, tmp_path):
    """rtx_render on an OBJ whose MTL names a PPM norm: differs from --no-normal-maps, equals the Python path's image; --bump-height on a PGM is the image of binding the
    twin's converted bytes"""
    from test_cutout_ref import write_card
    from test_denoise import read_exr_rgb
    rng = np.random.default_rng(8)
    rgb = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    grey = rng.integers(0, 256, (5, 9), dtype=np.uint8)
    (tmp_path / "n.ppm").write_bytes(b"P6 7 6 255\n" + rgb.tobytes())
    (tmp_path / "h.pgm").write_bytes(b"P5 9 5 255\n" + grey.tobytes())
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
    p = rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0)

    def cli(files, name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run([exe, "--obj", files[0], "--mtl", str(tmp_path), "--w", str(W), "--h", str(H), "--spp", "4", "--gpus", "1", "--out", out] + list(extra),
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out)

    def python(scene):
        c = rt.Context(0)
        c.upload(scene, W / H); c.clear(W, H); c.render(p)
        a = c.read_accum(); c.close()
        return a[..., :3] / np.maximum(a[..., 3:], np.float32(1.0))

    files, mtl = write_card(tmp_path, "norm n.ppm\n")
    sc = rt.Scene.from_obj(files, mtl)
    assert sc.normal_maps == [-1, -1, 0, -1]
    mapped = python(sc)
    sc.normal_maps = []
    plain = python(sc)
    assert not np.array_equal(bits(mapped), bits(plain)) and mapped.sum() > 0
    assert np.array_equal(bits(cli(files, "m.exr")), bits(mapped))
    assert np.array_equal(bits(cli(files, "p.exr", "--no-normal-maps")), bits(plain))
    assert np.array_equal(bits(cli(files, "t.exr", "--no-textures")), bits(plain))
    flipped = python(rt.Scene.from_obj(files, mtl, flip_y=True))
    assert np.array_equal(bits(cli(files, "f.exr", "--normal-flip-y")), bits(flipped)) and not np.array_equal(bits(flipped), bits(mapped))
    # a height map: the CLI's conversion is the twin's
    files, mtl = write_card(tmp_path, "map_Bump h.pgm\n")
    sc = rt.Scene.from_obj(files, mtl)
    assert sc.normal_maps == [-1, -1, -1, -1]
    h4 = np.dstack([grey, grey, grey, np.full_like(grey, 255)])
    sc.texture_pixels[0] = nr.height_to_normal(h4, 4.0); sc.normal_maps = [-1, -1, 0, -1]
    bumped = python(sc)
    assert np.array_equal(bits(cli(files, "b.exr", "--bump-height", "4")), bits(bumped)) and not np.array_equal(bits(bumped), bits(plain))
    assert np.array_equal(bits(cli(files, "q.exr")), bits(plain))             # map_Bump is used on request only

"""Diffuse texture maps on the device (include/rtx.h: rtx_set_mesh_uvs / rtx_set_texture / rtx_set_material_map), every check bit-exact:
the sampler and the per-hit albedo against the numpy emulation (tests/texture_ref.py), the transport against the ORACLE rendering the equivalent untextured scene — a texture
that is constant over each triangle is the scene whose triangles carry materials with Kd = Kd' — and the plumbing (commits, options, partners, errors) against itself."""
import os
import subprocess

import numpy as np
import pytest

import texture_ref as tr
from test_deform import ArrayScene, bits, place, random_rays, sine_deform

W, H = 96, 64
PT = dict(width=W, height=H, spp=4, max_bounces=5, nee_samples=2, rr_start=2)
ATRIUM, MONKE = 0, 1
MISS = np.uint32(0xFFFFFFFF)
GLASS = 14                      # the monkey's material: dissolve 0.5, Ni 1.5, mapped
LAMP = 12                       # the atrium's emitter, mapped (a map on an emitter has no effect)
SIZES = [(1, 1), (20, 48), (64, 64)]          # (H, W): 1 x 1; 48 x 20, non-square and no power of two; 64 x 64
SRGB = [False, True, False]
MAPS = {LAMP: 0, 9: 0, 1: 1, 3: 1, 5: 1, 7: 1, 2: 2, 4: 2, 6: 2, GLASS: 2}      # materials 0, 8, 10, 11, 13 stay unmapped


class TexScene(ArrayScene):
    """ArrayScene + the optional texture attributes Context.upload binds: uvs (per mesh), textures [(pixels, srgb)], material_maps (per material)"""
    def __init__(self, base, uvs=None, textures=None, material_maps=None):
        super().__init__(base.materials, base.meshes, base.instances, base._vp, base.lo, base.hi)
        self.uvs, self.textures, self.material_maps = uvs, textures, material_maps


def block_texture(rng, h, w):
    """a grid of 8 x 8-texel blocks of one colour each (the last row / column of blocks cropped where the size is no multiple of 8)"""
    cols = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8, 4), dtype=np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(cols, 8, 0), 8, 1)[:h, :w])


def noise_texture(rng, h, w):
    return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)


def block_uvs(rng, matids, maps):
    """per corner (index count, 2): the three corners of a triangle whose material maps to an image with whole 8 x 8 blocks lie in ONE such block, 1.5 texels inside it,
    shifted by a whole number of repeats; every other triangle gets anything in [-2, 3]^2"""
    ntri = len(matids) // 3
    uv = rng.uniform(-2.0, 3.0, (ntri, 3, 2))
    tex = np.array([maps.get(int(m), -1) for m in matids[0::3]])
    for k, (h, w) in enumerate(SIZES):
        sel = np.nonzero(tex == k)[0]
        if h < 8 or w < 8 or not len(sel):
            continue
        bx, by = rng.integers(0, w // 8, len(sel)), rng.integers(0, h // 8, len(sel))
        px = 8.0 * bx[:, None] + 1.5 + 5.0 * rng.random((len(sel), 3))
        py = 8.0 * by[:, None] + 1.5 + 5.0 * rng.random((len(sel), 3))
        uv[sel, :, 0] = px / w + rng.integers(-1, 2, len(sel))[:, None]
        uv[sel, :, 1] = 1.0 - py / h + rng.integers(-1, 2, len(sel))[:, None]
    return uv.reshape(-1, 2).astype(np.float32)


def tri_tables(sc):
    """per GLOBAL triangle id (instances in order, each the triangles of its mesh): material id, corner UVs (n, 3, 2)"""
    mats = [np.asarray(m, np.uint32)[0::3] for _, _, m in sc.meshes]
    mat = np.concatenate([mats[mesh] for mesh, _ in sc.instances])
    uv = np.concatenate([np.asarray(sc.uvs[mesh], np.float32).reshape(-1, 3, 2) for mesh, _ in sc.instances])
    return mat, uv


def expected_albedo(rt, sc, hits):
    """(n, 4) float32 as Context.albedo returns it, from the emulation"""
    mat, uv = tri_tables(sc)
    prim = hits[:, 3].view(np.uint32)
    out = np.zeros((len(hits), 4), np.float32)
    out[:, 3].view(np.uint32)[:] = MISS
    hit = np.nonzero(prim != MISS)[0]
    m = mat[prim[hit]]
    kd = tr.half_round_array(rt.half_round, np.asarray(sc.materials, np.float32)[m][:, :3])
    maps = np.array([-1 if t is None else t for t in sc.material_maps], np.int64)
    tex = maps[m]
    s, t = tr.interp_uv(uv[prim[hit]], hits[hit, 1], hits[hit, 2])
    for k, (px, srgb) in enumerate(sc.textures):
        sel = tex == k
        if sel.any():
            kd[sel] = tr.kd_prime(rt.half_round, np.asarray(sc.materials, np.float32)[m[sel]][:, :3], tr.sample(px, srgb, s[sel], t[sel]))
    out[hit, :3] = kd
    out[:, 3].view(np.uint32)[hit] = tex.astype(np.int32).view(np.uint32)
    return out


def equivalent(rt, sc):
    """the untextured scene a block-textured one is equal to: every triangle of a mapped material gets a material of its own kind with Kd = Kd' (one appended per distinct
    (material, value the triangle sees)); asserts with the emulation that all four taps agree at every corner of such a triangle"""
    materials = [np.array(m, np.float32) for m in np.asarray(sc.materials, np.float32)]
    made, meshes = {}, []
    for (v, i, mid), uv in zip(sc.meshes, sc.uvs):
        mid = np.array(mid, np.uint32, copy=True)
        uv3 = np.asarray(uv, np.float32).reshape(-1, 3, 2)
        tmat = mid[0::3].copy()
        for k, (px, srgb) in enumerate(sc.textures):
            sel = np.nonzero(np.array([sc.material_maps[m] == k for m in tmat]))[0]
            if not len(sel):
                continue
            for c in range(3):
                assert tr.taps_agree(px, uv3[sel, c, 0], uv3[sel, c, 1]).all()
            tl = tr.sample(px, srgb, uv3[sel, 0, 0], uv3[sel, 0, 1])
            for c in (1, 2):
                assert np.array_equal(bits(tr.sample(px, srgb, uv3[sel, c, 0], uv3[sel, c, 1])), bits(tl))
            kd = tr.kd_prime(rt.half_round, np.asarray(sc.materials, np.float32)[tmat[sel]][:, :3], tl)
            for t, m, q in zip(sel, tmat[sel], kd):
                key = (int(m), q.tobytes())
                if key not in made:
                    made[key] = len(materials)
                    nm = materials[int(m)].copy(); nm[0:3] = q
                    materials.append(nm)
                mid[3 * t:3 * t + 3] = made[key]
        meshes.append((v, i, mid))
    return ArrayScene(np.array(materials, np.float32), meshes, sc.instances, sc._vp, sc.lo, sc.hi)


def make_general(rt, golden_dir):
    """a ~4000-triangle atrium (13 materials, the last one its emitter) and monke.obj instanced twice, once mirrored and non-uniformly scaled: 5976 triangles, above the GPU
    builder's threshold.  The monkey's material is a dielectric (dissolve 0.5, Ni 1.5) with a diffuse share"""
    big = rt.Scene.sponza_class(4000, 260)
    small = rt.Scene.from_obj([os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    nm = len(big.materials)
    materials = np.concatenate([np.asarray(big.materials, np.float32), np.asarray(small.materials, np.float32)])
    assert nm == 13 and len(materials) == 15 and materials[LAMP, 8:11].sum() > 0
    materials[GLASS, 3], materials[GLASS, 7], materials[GLASS, 13] = 0.5, 1.5, 0.2
    meshes = list(big.meshes)
    base = sum(len(m) for _, _, m in big.meshes)
    v, i, m = small.meshes[0]
    v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)
    meshes.append((v, i, np.asarray(m, np.uint32) + np.uint32(nm)))
    assert set(np.unique(meshes[MONKE][2])) == {GLASS}
    instances = list(big.instances) + [(MONKE, place(0.0, 0.3, 0.0, 0.25, 0.25, 0.25)), (MONKE, place(0.8, 0.5, 0.2, -0.45, 0.3, 0.35))]
    return ArrayScene(materials, meshes, instances, big.view_proj, -1.5, 1.5), big


class World:
    """the two scenes of this module in their block-textured and noise-textured forms, and what the oracle says about the equivalent untextured scenes (each rendered once)"""
    def __init__(self, rt, orc, golden_dir):
        self.rt, self.orc = rt, orc
        rng = np.random.default_rng(20261019)
        self.plain, self._keep = make_general(rt, golden_dir)
        maps = [MAPS.get(m, -1) for m in range(len(self.plain.materials))]
        self.block_tex = [(block_texture(rng, h, w), s) for (h, w), s in zip(SIZES, SRGB)]
        self.noise_tex = [(noise_texture(rng, h, w), s) for (h, w), s in zip(SIZES, SRGB)]
        self.block_uvs = [block_uvs(rng, m, MAPS) for _, _, m in self.plain.meshes]
        self.free_uvs = [rng.uniform(-2.0, 3.0, (len(m), 2)).astype(np.float32) for _, _, m in self.plain.meshes]
        self.blocks = TexScene(self.plain, self.block_uvs, self.block_tex, maps)
        self.noise = TexScene(self.plain, self.free_uvs, self.noise_tex, maps)
        mv, mi, _ = self.plain.meshes[MONKE]
        self.monke2 = sine_deform(mv, mi, 0.06, 9.0, 0.0)
        edited = self.plain.with_meshes([(MONKE, self.monke2)])
        edited.instances = edited.instances[:2]                  # (the hidden instance is the last one: ids keep their meaning)
        self.edited = TexScene(edited, self.block_uvs, self.block_tex, maps)
        self.cornell = rt.Scene.cornell()
        cmaps = {2: 1, 3: 2}                                     # the red and the green wall
        cb = ArrayScene(self.cornell.materials, self.cornell.meshes, self.cornell.instances, self.cornell.view_proj, -1.0, 1.0)
        self.tiny_plain = cb
        self.tiny = TexScene(cb, [block_uvs(rng, m, cmaps) for _, _, m in cb.meshes], self.block_tex, [cmaps.get(m, -1) for m in range(len(cb.materials))])
        self._oracle = {}

    def expect(self, name, flags):
        """oracle image and ray counts of the untextured equivalent of scene `name` under `flags`"""
        key = (name, flags)
        if key not in self._oracle:
            o = self.orc.Oracle().load(equivalent(self.rt, getattr(self, name)), W / H)
            self._oracle[key] = o.render(self.rt.Params(flags=flags, **PT))
            o.close()
        return self._oracle[key]


@pytest.fixture(scope="module")
def world(rt, orc, golden_dir):
    return World(rt, orc, golden_dir)


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


def check_transport(rt, c, world, name, flags, tag):
    acc, cnt = world.expect(name, flags)
    img, st = frame(rt, c, flags), c.stats()
    assert np.array_equal(bits(img), bits(acc)), tag
    assert (st.rays_primary, st.rays_extension, st.rays_shadow) == cnt, tag
    return st


# ------------------------------------------------------------------------------------------------
# 1. the sampler
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sampler_to_the_bit(rt, world):
    """Context.texture_sample == the emulation on every texture and both encodings: 4096 UVs in [-2, 3]^2, every texel centre, every texel edge, 0 and 1 exactly"""
    c = context(rt, [], world.noise)
    rng = np.random.default_rng(5)
    for k, (px, srgb) in enumerate(world.noise_tex):
        h, w = px.shape[:2]
        cx, cy = np.meshgrid((np.arange(w) + 0.5) / w, (np.arange(h) + 0.5) / h)
        ex, ey = np.meshgrid(np.arange(w + 1) / w, np.arange(h + 1) / h)
        uv = np.concatenate([rng.uniform(-2.0, 3.0, (4096, 2)), np.stack([cx.ravel(), cy.ravel()], 1), np.stack([ex.ravel(), ey.ravel()], 1),
                             np.stack([ex.ravel() - 1.0, ey.ravel() + 2.0], 1), [[0, 0], [1, 1], [0, 1], [1, 0], [-0.0, 1.0], [-1e-9, 1e-9]]]).astype(np.float32)
        got = c.texture_sample(k, uv)
        assert np.array_equal(bits(got[:, :3]), bits(tr.sample(px, srgb, uv[:, 0], uv[:, 1]))), k
        assert not got[:, 3].any()
    c.close()


# ------------------------------------------------------------------------------------------------
# 2. the albedo at hits
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_albedo_at_hits_to_the_bit(rt, orc, world):
    """noise textures, free UVs: Context.albedo at the oracle's hits (camera rays + 4096 random rays) == the emulation, and debug layer 13 == its packed form"""
    sc = world.noise
    o = orc.Oracle().load(sc, W / H)
    cam = o.primary_rays(rt.Params(width=W, height=H))
    rays = np.concatenate([cam, random_rays(4096, 17, sc.lo, sc.hi)])
    hits = o.trace_closest(rays, 1)
    o.close()
    want = expected_albedo(rt, sc, hits)
    prim = hits[:, 3].view(np.uint32)
    texid = want[prim != MISS, 3].view(np.int32)
    assert all((texid == k).sum() > 50 for k in (-1, 0, 1, 2)) and (prim == MISS).any()          # every kind of hit is there
    c = context(rt, [], sc)
    assert np.array_equal(bits(c.albedo(hits, rays)), bits(want))
    assert np.array_equal(bits(c.albedo(hits)), bits(want))
    layer = c.read_layer(13, W, H).reshape(-1, 4)
    exp = tr.pack_rgb8(want[:W * H, :3])
    assert np.array_equal(layer, exp)
    # a context without maps shows the materials' own colour
    p = context(rt, [], world.plain)
    flat = p.albedo(hits)
    assert (flat[:, 3].view(np.uint32) == MISS).all()
    unm = texid == -1
    assert np.array_equal(bits(flat[prim != MISS][unm]), bits(want[prim != MISS][unm])) and not np.array_equal(p.read_layer(13, W, H).reshape(-1, 4), layer)
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 3. transport
# ------------------------------------------------------------------------------------------------
CONFIGS = {"default": [], "state_by_path": [("OPT_COMPACT_STATE", 0)], "gpu_build": [("OPT_GPU_BUILD", 1)],
           "ignored_variants": [("OPT_FUSED_BVH", 1), ("OPT_SHADE_DENSE", 1), ("OPT_SORT_MATERIALS", 1)]}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_block_textures_equal_per_triangle_materials(rt, world, config):
    """block textures: read_accum == the oracle's image of the equivalent untextured scene, for default flags, RTX_FLAG_LAMBERT_ONLY and RTX_FLAG_TRANSMISSION"""
    c = context(rt, CONFIGS[config], world.blocks)
    for flags in (0, rt.FLAG_LAMBERT_ONLY, rt.FLAG_TRANSMISSION):
        st = check_transport(rt, c, world, "blocks", flags, (config, flags))
        assert st.kernel_launches[rt.K_SHADE] > 0 and st.kernel_launches[rt.K_BOUNCE] == 0      # the separate kernels, whatever the options say
    if config == "gpu_build":
        assert c.build_info()["clusters_top"] > 0                  # built on the device
    c.close()


@pytest.mark.gpu
def test_block_textures_two_shards(rt, world):
    c = context(rt, [], world.blocks)
    acc, _ = world.expect("blocks", 0)
    c.clear(W, H)
    for r in range(2):
        c.render(rt.Params(tile_size=16, shard_rank=r, shard_count=2, **PT))
    assert np.array_equal(bits(c.read_accum()), bits(acc))
    c.close()


@pytest.mark.gpu
def test_block_textures_tiny_scene(rt, world):
    """the Cornell box with maps on two walls runs on the general path and equals the oracle's equivalent"""
    c = context(rt, [], world.tiny)
    for flags in (0, rt.FLAG_LAMBERT_ONLY):
        st = check_transport(rt, c, world, "tiny", flags, flags)
        assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] > 0
    c.close()


# ------------------------------------------------------------------------------------------------
# 4. invariance
# ------------------------------------------------------------------------------------------------
def bind(c, sc, maps=True):
    for mesh, uv in enumerate(sc.uvs):
        c.set_mesh_uvs(mesh, uv)
    for k, (px, srgb) in enumerate(sc.textures):
        c.set_texture(k, px, srgb)
    if maps:
        for m, t in enumerate(sc.material_maps):
            c.set_material_map(m, t)


@pytest.mark.gpu
def test_invariance_general(rt, world):
    """UVs and textures without a map change nothing; mapping changes the image; unmapping restores it — and none of these commits touches the tree"""
    c = context(rt, [], world.plain)
    base, tree, refits = frame(rt, c), c.tree_hash(), c.stats().bvh_refits
    bind(c, world.blocks, maps=False)
    with pytest.raises(rt.RtxError):
        c.render(rt.Params(**PT))                                # edits need a commit
    c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and (c.tree_hash(), c.stats().bvh_refits) == (tree, refits)
    bind(c, world.blocks); c.commit()
    mapped = frame(rt, c)
    assert not np.array_equal(bits(mapped), bits(base)) and (c.tree_hash(), c.stats().bvh_refits) == (tree, refits)
    assert np.array_equal(bits(mapped), bits(world.expect("blocks", 0)[0]))
    for m in range(len(world.plain.materials)):
        c.set_material_map(m, -1)
    c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and (c.tree_hash(), c.stats().bvh_refits) == (tree, refits)
    c.close()


@pytest.mark.gpu
def test_invariance_tiny(rt, world):
    """the tiny scene leaves the fused path while a map is active and is back on it, with its image, afterwards"""
    c = context(rt, [], world.tiny_plain)
    base = frame(rt, c)
    assert c.stats().kernel_launches[rt.K_BOUNCE] > 0
    bind(c, world.tiny, maps=False); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and c.stats().kernel_launches[rt.K_BOUNCE] > 0
    bind(c, world.tiny); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(world.expect("tiny", 0)[0])) and c.stats().kernel_launches[rt.K_BOUNCE] == 0
    for m in range(len(world.tiny.materials)):
        c.set_material_map(m, -1)
    c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and c.stats().kernel_launches[rt.K_BOUNCE] > 0
    c.close()


# ------------------------------------------------------------------------------------------------
# 5. edits
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", ["default", "gpu_build"])
def test_maps_stay_on_their_triangles_through_edits(rt, world, config):
    """new vertices for the monkey and its second instance hidden, in one commit: the image is the oracle's of the equivalent edited scene"""
    c = context(rt, CONFIGS[config], world.blocks)
    c.update_mesh_vertices(MONKE, world.monke2)
    c.set_instance_visible(2, False)
    c.commit()
    check_transport(rt, c, world, "edited", 0, config)
    c.close()


# ------------------------------------------------------------------------------------------------
# 6. partners
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adaptive_and_denoise_guides(rt, world):
    """render_adaptive with threshold 0 == render on the textured scene; the denoiser's guides do not see maps"""
    c = context(rt, [], world.noise)
    ref = frame(rt, c)
    c.clear(W, H)
    c.render_adaptive(rt.Params(**PT), 2, 2, PT["spp"], 0.0)
    assert np.array_equal(bits(c.read_accum()), bits(ref))
    guides = c.denoise_guides(W, H)
    p = context(rt, [], world.plain)
    assert np.array_equal(bits(p.denoise_guides(W, H)), bits(guides))
    assert not np.array_equal(bits(frame(rt, p)), bits(ref))
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 7. errors and state
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_the_scene_committed(rt, world, tmp_path):
    sc = world.blocks
    c = context(rt, [], sc)
    ref = frame(rt, c)
    L, nidx = rt.lib, len(sc.meshes[MONKE][1])
    uv = np.ascontiguousarray(sc.uvs[MONKE]); px = np.zeros((4, 4, 4), np.uint8)
    bad = uv.copy(); bad[7, 1] = np.inf
    nan = uv.copy(); nan[0, 0] = np.nan
    P = lambda a: a.ctypes.data_as(rt.C.c_void_p)
    calls = [lambda: L.rtx_set_mesh_uvs(c._h, 9, P(uv), nidx), lambda: L.rtx_set_mesh_uvs(c._h, MONKE, P(uv), nidx - 3), lambda: L.rtx_set_mesh_uvs(c._h, MONKE, P(bad), nidx),
             lambda: L.rtx_set_mesh_uvs(c._h, MONKE, P(nan), nidx),
             lambda: L.rtx_set_texture(c._h, 4, P(px), 4, 4, 0), lambda: L.rtx_set_texture(c._h, 0, P(px), 0, 4, 0), lambda: L.rtx_set_texture(c._h, 0, P(px), 4, 16385, 0),
             lambda: L.rtx_set_texture(c._h, 0, P(px), 4, 4, 2), lambda: L.rtx_set_texture(c._h, 0, None, 4, 4, 0),
             lambda: L.rtx_set_material_map(c._h, 15, rt.MAP_KD, 0), lambda: L.rtx_set_material_map(c._h, 1, 1, 0), lambda: L.rtx_set_material_map(c._h, 1, rt.MAP_KD, 3),
             lambda: L.rtx_set_material_map(c._h, 1, rt.MAP_KD, -2)]
    for k, call in enumerate(calls):
        assert call() == -1, k                                   # RTX_ERR_INVALID
        assert np.array_equal(bits(frame(rt, c)), bits(ref)), k  # ... untouched, and still committed
    assert L.rtx_debug_texture_sample(c._h, 3, P(uv), 1, P(np.zeros(4, np.float32))) == -1
    hits = np.zeros((1, 4), np.float32); hits[0, 3:].view(np.uint32)[:] = c.stats().triangles
    assert L.rtx_debug_albedo(c._h, None, P(hits), 1, P(np.zeros(4, np.float32))) == -1
    # a scene cache holds no texels
    assert L.rtx_save_scene_cache(c._h, str(tmp_path / "t.rtxscn").encode()) == -4               # RTX_ERR_STATE
    # a setter un-commits
    c.set_material_map(1, 2)
    assert L.rtx_render(c._h, rt.C.byref(rt.Params(**PT))) == -4
    c.set_material_map(1, 1); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(ref))
    # rtx_set_materials replaces the table: no material has a map afterwards, and the cache can be written again
    c.set_materials(sc.materials); c.commit()
    p = context(rt, [], world.plain)
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, p)))
    c.save_scene_cache(tmp_path / "t.rtxscn")
    # NULL clears a mesh's UVs: every corner is (0, 0)
    bind(c, sc); c.set_mesh_uvs(MONKE, None); c.commit()
    z = TexScene(world.plain, [sc.uvs[ATRIUM], np.zeros_like(sc.uvs[MONKE])], sc.textures, sc.material_maps)
    q = context(rt, [], z)
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, q)))
    # a loaded cache has no maps
    c.load_scene_cache(tmp_path / "t.rtxscn"); c.set_camera(*world.plain.view_proj(W / H))
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, p)))
    q.close(); p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 8. the C++ host layer and the CLI
# ------------------------------------------------------------------------------------------------
ROOM_OBJ = """mtllib room.mtl
v -2 0 -1
v 2 0 -1
v 2 3 -1
v -2 3 -1
v -2 0 3
v 2 0 3
v -0.5 2.9 0.5
v 0.5 2.9 0.5
v 0.5 2.9 1.5
v -0.5 2.9 1.5
vt 0 0
vt 2 0
vt 2 1.5
vt 0 1.5
usemtl wall
f 1/1 2/2 3/3 4/4
usemtl floor
f 5/1 6/2 2/3 1/4
usemtl lamp
f 7 10 9 8
"""
ROOM_MTL = "newmtl wall\nKd 0.9 0.9 0.9\nmap_Kd wall.ppm\nnewmtl floor\nKd 0.8 0.8 0.8\nmap_Kd floor.tga\nnewmtl lamp\nKd 0 0 0\nKe 12 11 10\n"


@pytest.mark.gpu
def test_cli_renders_map_kd(rt, tmp_path):
    """rtx_render on an OBJ whose MTL names a P6 and a TGA == the Python path's image of the same files, on one context and on the native two-rank frame;
    --no-textures == the scene without maps"""
    from test_denoise import read_exr_rgb
    from test_texture_ref import tga_bytes
    rng = np.random.default_rng(8)
    wall = np.repeat(np.repeat(rng.integers(0, 256, (6, 8, 3), dtype=np.uint8), 4, 0), 4, 1)
    floor = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    (tmp_path / "wall.ppm").write_bytes(b"P6 32 24 255\n" + wall.tobytes())
    (tmp_path / "floor.tga").write_bytes(tga_bytes(floor, 24, False, True))
    (tmp_path / "room.mtl").write_text(ROOM_MTL)
    (tmp_path / "room.obj").write_text(ROOM_OBJ)
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
    base = [exe, "--obj", str(tmp_path / "room.obj"), "--mtl", str(tmp_path), "--w", str(W), "--h", str(H), "--spp", "4"]

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out", out] + list(extra), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out)

    sc = rt.Scene.from_obj([str(tmp_path / "room.obj")], str(tmp_path) + "/")
    assert [None if t is None else t.shape for t in sc.texture_pixels] == [(24, 32, 4), (16, 16, 4)]
    p = rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0)

    def python(scene):
        c = rt.Context(0)
        c.upload(scene, W / H); c.clear(W, H); c.render(p)
        a = c.read_accum(); c.close()
        return a[..., :3] / np.maximum(a[..., 3:], np.float32(1.0))

    textured = python(sc)
    sc.material_maps = []
    plain = python(sc)
    assert not np.array_equal(bits(textured), bits(plain)) and textured.sum() > 0
    assert np.array_equal(bits(cli("t.exr")), bits(textured))
    assert np.array_equal(bits(cli("n.exr", "--no-textures")), bits(plain))
    assert np.array_equal(bits(cli("t2.exr", "--gpus", "2", "--devices", "0,0", "--gather", "copy")), bits(textured))

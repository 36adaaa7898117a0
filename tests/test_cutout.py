"""Alpha cut-outs on the device (include/rtx.h: ALPHA CUT-OUTS), every comparison bit-exact: the probe against the numpy twin (tests/cutout_ref.py); hit records with partial
alpha against the oracle's hits combined with the twin's verdicts; the transport against the ORACLE rendering the equivalent scene — a scene in which every cut-out triangle
sees alpha on one side of 0.5 is the scene in which the rejected triangles do not exist (here: are degenerate, i1 = i2 = i0, so that ids keep their meaning) — and the plumbing
(commits, options, partners, errors, the command line) against itself."""
import os
import subprocess

import numpy as np
import pytest

import cutout_ref as cr
from test_deform import ArrayScene, bits, random_rays, sine_deform
from test_texture import GLASS, LAMP, MISS, PT, SIZES, SRGB, H, W, TexScene, bind, block_texture, block_uvs, equivalent, make_general, noise_texture

ATRIUM, MONKE, CARDS, MONKE2 = 0, 1, 2, 3            # meshes; the instances are in the same order, MONKE2's last (hiding it keeps every other id)
GLASS2, CARD = 15, 16                                # materials of their own: the second monkey's mesh, the two card grids
OPAC = {1: 1, 3: 2, 5: 1, 9: 0, LAMP: 1, GLASS: 2, CARD: 2}      # material -> opacity texture; the lamp's has no effect (an emitter)
NCARD = 32


class CutScene(TexScene):
    """TexScene + opacity_maps (per material), which Context.upload binds like material_maps"""
    def __init__(self, base, uvs, textures, material_maps, opacity_maps):
        super().__init__(base, uvs, textures, material_maps)
        self.opacity_maps = opacity_maps


def card_mesh(base, mat):
    """two 4 x 2 quad grids (32 triangles) in the unit square of the xy plane at z = 0 and z = 1"""
    v, idx = [], []
    for z in (0.0, 1.0):
        o = len(v)
        for j in range(3):
            for i in range(5):
                v.append([i / 4.0 - 0.5, j / 2.0 - 0.5, z, 0.0, 0.0, 1.0, float(base)])
        for j in range(2):
            for i in range(4):
                q = o + j * 5 + i
                idx += [q, q + 1, q + 6, q, q + 6, q + 5]
    return np.array(v, np.float32), np.array(idx, np.uint32), np.full(len(idx), mat, np.uint32)


def look_from(eye, center, dist, depth, width, height, yaw):
    """the 16-float matrix (row-vector convention) that puts card_mesh's unit square at `dist` along eye -> center, facing the eye and turned by yaw about the up axis; its
    z = 1 grid lies `depth` farther away"""
    f = (center - eye) / np.linalg.norm(center - eye)
    r = np.cross(f, [0.0, 1.0, 0.0]); r /= np.linalg.norm(r)
    u = np.cross(r, f)
    cs, sn = np.cos(yaw), np.sin(yaw)
    r2, f2 = cs * r + sn * f, cs * f - sn * r
    m = np.eye(4)
    m[0, :3], m[1, :3], m[2, :3], m[3, :3] = width * r2, height * u, depth * f2, eye + dist * f
    return m.astype(np.float32).reshape(16)


def block_alpha(tex):
    """alpha 0 or 255 per 8 x 8 block (the colour stays one value per block)"""
    out = tex.copy(); out[..., 3] = np.where(tex[..., 3] < 128, 0, 255)
    return out


def degenerate(sc, rejected):
    """sc with the triangles rejected[mesh] (bool per triangle) made degenerate: i1 = i2 = i0"""
    meshes = []
    for (v, i, m), rej in zip(sc.meshes, rejected):
        i = np.array(i, np.uint32, copy=True).reshape(-1, 3)
        i[rej, 1] = i[rej, 0]; i[rej, 2] = i[rej, 0]
        meshes.append((v, i.reshape(-1), m))
    return ArrayScene(sc.materials, meshes, sc.instances, sc._vp, sc.lo, sc.hi)


def rejected_triangles(sc):
    """per mesh: the triangles whose alpha is rejected over their whole area; asserts with the twin that the four taps agree at every corner of every cut-out triangle"""
    out, ncut = [], 0
    for (v, i, mid), uv in zip(sc.meshes, sc.uvs):
        tex = cr.cut_textures(sc.materials, sc.opacity_maps, np.asarray(mid, np.uint32)[0::3])
        uv3 = np.asarray(uv, np.float32).reshape(-1, 3, 2)
        rej = np.zeros(len(tex), bool)
        for k, (px, _) in enumerate(sc.textures):
            sel = np.nonzero(tex == k)[0]
            if not len(sel):
                continue
            ok = [cr.accepted(cr.alpha(px, uv3[sel, c, 0], uv3[sel, c, 1])) for c in range(3)]
            for c in range(3):
                assert cr.alpha_taps_agree(px, uv3[sel, c, 0], uv3[sel, c, 1]).all()
            assert np.array_equal(ok[0], ok[1]) and np.array_equal(ok[0], ok[2])
            rej[sel] = ~ok[0]; ncut += len(sel)
        out.append(rej)
    return out, ncut


def cut_equivalent(rt, sc):
    """the scene without maps a block-mapped one is equal to: Kd' materials for the diffuse maps (test_texture.equivalent), rejected triangles degenerate"""
    rej, ncut = rejected_triangles(sc)
    nrej = sum(int(r.sum()) for r in rej)
    assert 0 < nrej < ncut                                          # both verdicts occur
    base = equivalent(rt, sc) if any(t is not None and t >= 0 for t in sc.material_maps) else sc
    return degenerate(base, rej)


def tri_tables(sc):
    """per GLOBAL triangle id: material id, corner UVs (n, 3, 2), opacity texture or -1"""
    mats = [np.asarray(m, np.uint32)[0::3] for _, _, m in sc.meshes]
    mat = np.concatenate([mats[mesh] for mesh, _ in sc.instances])
    uv = np.concatenate([np.asarray(sc.uvs[mesh], np.float32).reshape(-1, 3, 2) for mesh, _ in sc.instances])
    return mat, uv, cr.cut_textures(sc.materials, sc.opacity_maps, mat)


class World:
    def __init__(self, rt, orc, golden_dir):
        self.rt, self.orc = rt, orc
        rng = np.random.default_rng(20261020)
        g, self._keep = make_general(rt, golden_dir)
        eye, center = np.asarray(self._keep.eye, np.float64), np.asarray(self._keep.center, np.float64)
        materials = np.concatenate([np.asarray(g.materials, np.float32), np.asarray(g.materials, np.float32)[[GLASS, 5]]])
        meshes = list(g.meshes)
        base = sum(len(m) for _, _, m in meshes)
        meshes.append(card_mesh(base, CARD)); base += len(meshes[-1][2])
        v, i, m = g.meshes[MONKE]
        v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)
        meshes.append((v, i, np.full(len(m), GLASS2, np.uint32)))
        d = float(np.linalg.norm(center - eye))
        self.card_o2w = look_from(eye, center, 0.30 * d, 0.25 * d, 0.55 * d, 0.35 * d, 0.5)
        self.card_o2w2 = look_from(eye, center, 0.35 * d, 0.15 * d, 0.45 * d, 0.40 * d, -0.4)
        instances = list(g.instances[:-2]) + [g.instances[-2], (CARDS, self.card_o2w), (MONKE2, g.instances[-1][1])]
        assert [mesh for mesh, _ in instances] == [ATRIUM, MONKE, CARDS, MONKE2]
        self.plain = ArrayScene(materials, meshes, instances, g._vp, g.lo, g.hi)
        nmat = len(materials)
        omaps = [OPAC.get(m, -1) for m in range(nmat)]
        none = [-1] * nmat
        self.block_tex = [(block_alpha(block_texture(rng, h, w)), s) for (h, w), s in zip(SIZES, SRGB)]
        self.block_tex[0][0][..., 3] = 0                            # the 1 x 1 texture: everything it covers is cut away
        self.noise_tex = [(noise_texture(rng, h, w), s) for (h, w), s in zip(SIZES, SRGB)]
        self.block_uvs = [block_uvs(rng, m, OPAC) for _, _, m in meshes]
        self.free_uvs = [rng.uniform(-2.0, 3.0, (len(m), 2)).astype(np.float32) for _, _, m in meshes]
        self.cut = CutScene(self.plain, self.block_uvs, self.block_tex, none, omaps)                  # cut-outs and NO map_Kd anywhere
        self.both = CutScene(self.plain, self.block_uvs, self.block_tex, omaps, omaps)                # the same texture serves both slots of every mapped material
        self.noise = CutScene(self.plain, self.free_uvs, self.noise_tex, [(-1 if m % 2 else t) for m, t in enumerate(omaps)], omaps)
        cards_only = [(OPAC[CARD] if m == CARD else -1) for m in range(nmat)]
        self.cards = CutScene(self.plain, self.free_uvs, self.noise_tex, none, cards_only)
        # edits: the monkey deformed and the cards moved; then the second monkey hidden
        mv, mi, _ = meshes[MONKE]
        self.monke2 = sine_deform(mv, mi, 0.06, 9.0, 0.0)
        e1 = self.plain.with_meshes([(MONKE, self.monke2)])
        e1.instances = [instances[0], instances[1], (CARDS, self.card_o2w2), instances[3]]
        self.edited1 = CutScene(e1, self.block_uvs, self.block_tex, none, omaps)
        e2 = self.plain.with_meshes([(MONKE, self.monke2)])
        e2.instances = e1.instances[:3]
        self.edited2 = CutScene(e2, self.block_uvs, self.block_tex, none, omaps)
        # the Cornell box, its short box (triangles 12 .. 21) with a material of its own
        cb = rt.Scene.cornell()
        self._keep2 = cb
        cmat = np.concatenate([np.asarray(cb.materials, np.float32), np.asarray(cb.materials, np.float32)[[1]]])
        cv, ci, cm = cb.meshes[0]
        cm = np.array(cm, np.uint32, copy=True); cm[36:66] = 5
        self.tiny_plain = ArrayScene(cmat, [(cv, ci, cm)], cb.instances, cb.view_proj, -1.0, 1.0)
        self.tiny = CutScene(self.tiny_plain, [block_uvs(rng, cm, {5: 2})], self.block_tex, [-1] * 6, [-1, -1, -1, -1, -1, 2])
        self._oracle = {}

    def expect(self, name, flags):
        """oracle image and ray counts of the equivalent of scene `name` under `flags`"""
        key = (name, flags)
        if key not in self._oracle:
            sc = getattr(self, name)
            o = self.orc.Oracle().load(cut_equivalent(self.rt, sc) if isinstance(sc, CutScene) else sc, W / H)
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


def counts(c):
    st = c.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def check_transport(rt, c, world, name, flags, tag):
    acc, cnt = world.expect(name, flags)
    img = frame(rt, c, flags)
    assert np.array_equal(bits(img), bits(acc)), tag
    assert counts(c) == cnt, tag
    return c.stats()


def probe_rays(rt, o, sc, seed):
    cam = o.primary_rays(rt.Params(width=W, height=H))
    return np.concatenate([cam, random_rays(4096, seed, sc.lo, sc.hi)])


# ------------------------------------------------------------------------------------------------
# 1. the probe
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_probe_to_the_bit(rt, orc, world):
    """noise RGBA textures, free UVs: Context.opacity at the oracle's hits on the plain scene (camera rays + 4096 random rays) == the twin"""
    sc = world.noise
    o = orc.Oracle().load(world.plain, W / H)
    rays = probe_rays(rt, o, sc, 17)
    hits = o.trace_closest(rays, 1)
    o.close()
    mat, uv3, tcut = tri_tables(sc)
    want = cr.opacity_probe(sc.textures, tcut, uv3, hits)
    prim = hits[:, 3].view(np.uint32)
    texid = want[:, 1].view(np.uint32)
    assert ((prim != MISS) & (texid != MISS)).sum() > 200 and ((prim != MISS) & (texid == MISS)).sum() > 200 and (prim == MISS).sum() > 0      # every kind of hit
    assert (tcut[prim[prim != MISS]] == 0).any() and (mat[prim[prim != MISS]] == LAMP).any()                                                # the 1 x 1 texture; the emitter
    c = context(rt, [], sc)
    got = c.opacity(hits)
    assert np.array_equal(bits(got), bits(want))
    a = got[texid != MISS, 0]
    assert (a >= 0.5).any() and (a < 0.5).any()
    p = context(rt, [], world.plain)                                 # no cut-out active: (1, none) everywhere
    flat = p.opacity(hits)
    assert (flat[:, 0] == 1.0).all() and (flat[:, 1].view(np.uint32) == MISS).all()
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 2. hit records with partial alpha
# ------------------------------------------------------------------------------------------------
def expected_partial_hits(rt, orc, world):
    """rays, the expected closest-hit records, per ray whether a rejected candidate lies nearer than the expected hit, the number of accepted candidates"""
    sc = world.cards
    vc, ic, mc = sc.meshes[CARDS]
    tri_base = sum(len(sc.meshes[mesh][1]) // 3 for mesh, _ in sc.instances[:CARDS])
    rej = [np.zeros(len(i) // 3, bool) for _, i, _ in sc.meshes]; rej[CARDS][:] = True
    o = orc.Oracle().load(degenerate(world.plain, rej), W / H)
    rays = probe_rays(rt, o, sc, 23)
    best = o.trace_closest(rays, 1).copy()
    o.close()
    px = sc.textures[OPAC[CARD]][0]
    uv3 = np.asarray(sc.uvs[CARDS], np.float32).reshape(-1, 3, 2)
    v1 = np.array(vc, np.float32, copy=True); v1[:, 6] = 0.0
    rejected_t = np.full(len(rays), np.inf, np.float32)
    naccept = 0
    for k in range(NCARD):
        one = ArrayScene(sc.materials, [(v1, np.asarray(ic, np.uint32)[3 * k:3 * k + 3], np.asarray(mc, np.uint32)[3 * k:3 * k + 3])], [(0, world.card_o2w)], sc._vp, sc.lo, sc.hi)
        o1 = orc.Oracle().load(one, W / H)
        h = o1.trace_closest(rays, 1)
        o1.close()
        hit = h[:, 3].view(np.uint32) != MISS
        ok = np.zeros(len(rays), bool)
        ok[hit] = cr.accepted(cr.alpha_at(px, np.repeat(uv3[k:k + 1], hit.sum(), 0), h[hit, 1], h[hit, 2]))
        rejected_t[hit & ~ok] = np.minimum(rejected_t[hit & ~ok], h[hit & ~ok, 0])
        gid = np.uint32(tri_base + k)
        bp = best[:, 3].view(np.uint32)
        take = ok & ((h[:, 0] < best[:, 0]) | (bp == MISS) | ((h[:, 0] == best[:, 0]) & (gid < bp)))
        best[take, :3] = h[take, :3]
        best[:, 3].view(np.uint32)[take] = gid
        naccept += int(ok.sum())
    nearer_rejected = rejected_t < np.where(best[:, 3].view(np.uint32) == MISS, np.float32(np.inf), best[:, 0])
    return rays, best, nearer_rejected, naccept


@pytest.mark.gpu
def test_hits_with_partial_alpha(rt, orc, world):
    """32 cut-out triangles with a noise alpha map in an otherwise opaque scene: trace_closest == the oracle's hits on the scene without them, combined by (t, lower id) with the
    oracle's hit on each of the 32 triangles alone, filtered by the twin; trace_any == its existence form.  No exclusions: the definition leaves no tolerance"""
    rays, best, nearer_rejected, naccept = expected_partial_hits(rt, orc, world)
    assert nearer_rejected.sum() >= 200 and naccept >= 200, (int(nearer_rejected.sum()), naccept)      # or the test shows nothing
    c = context(rt, [], world.cards)
    got = c.trace_closest(rays)
    assert np.array_equal(bits(got), bits(best))
    assert np.array_equal(c.trace_any(rays), (best[:, 3].view(np.uint32) != MISS).astype(np.uint8))
    c.close()


# ------------------------------------------------------------------------------------------------
# 3. transport
# ------------------------------------------------------------------------------------------------
CONFIGS = {"default": [], "state_by_path": [("OPT_COMPACT_STATE", 0)], "gpu_build": [("OPT_GPU_BUILD", 1)],
           "sched_0": [("OPT_TRACE_SCHED", 0)], "sched_2": [("OPT_TRACE_SCHED", 2)], "sched_5": [("OPT_TRACE_SCHED", 5)],
           "stack_private": [("OPT_STACK_PRIVATE", 1)], "stack_overflow": [("OPT_STACK_CAP", 4)], "stack_overflow_sched_0": [("OPT_STACK_CAP", 4), ("OPT_TRACE_SCHED", 0)],
           "trace_counters": [("OPT_TRACE_COUNTERS", 1)],
           "ignored_variants": [("OPT_FUSED_BVH", 1), ("OPT_SHADE_DENSE", 1), ("OPT_SORT_MATERIALS", 1), ("OPT_WORK_STEALING", 1), ("OPT_OCCLUDER_CACHE", 1)]}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_block_alpha_equals_the_scene_without_the_rejected_triangles(rt, world, config):
    """block alpha maps, no map_Kd anywhere: read_accum and the three ray counts == the oracle's of the scene with the rejected triangles degenerate, for default flags,
    RTX_FLAG_LAMBERT_ONLY and RTX_FLAG_TRANSMISSION"""
    c = context(rt, CONFIGS[config], world.cut)
    for flags in (0, rt.FLAG_LAMBERT_ONLY, rt.FLAG_TRANSMISSION):
        st = check_transport(rt, c, world, "cut", flags, (config, flags))
        assert st.kernel_launches[rt.K_SHADE] > 0 and st.kernel_launches[rt.K_BOUNCE] == 0      # the separate kernels, whatever the options say
    if config == "gpu_build":
        assert c.build_info()["clusters_top"] > 0
    if config == "trace_counters":
        assert all(v > 0 for v in c.trace_counters())
    c.close()
    assert not np.array_equal(bits(world.expect("cut", 0)[0]), bits(world.expect("plain", 0)[0]))


@pytest.mark.gpu
def test_one_texture_in_both_slots(rt, world):
    c = context(rt, [], world.both)
    for flags in (0, rt.FLAG_LAMBERT_ONLY, rt.FLAG_TRANSMISSION):
        check_transport(rt, c, world, "both", flags, flags)
    c.close()
    assert not np.array_equal(bits(world.expect("both", 0)[0]), bits(world.expect("cut", 0)[0]))


# ------------------------------------------------------------------------------------------------
# 4. two shards, 5. the tiny scene
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_shards(rt, world):
    c = context(rt, [], world.cut)
    acc, _ = world.expect("cut", 0)
    c.clear(W, H)
    for r in range(2):
        c.render(rt.Params(tile_size=16, shard_rank=r, shard_count=2, **PT))
    assert np.array_equal(bits(c.read_accum()), bits(acc))
    c.close()


@pytest.mark.gpu
def test_tiny_scene(rt, world):
    """the Cornell box with a cut-out map on the short box's material runs on the general path and equals the oracle's equivalent; unbound, it is back on the fused path"""
    c = context(rt, [], world.tiny)
    for flags in (0, rt.FLAG_LAMBERT_ONLY):
        st = check_transport(rt, c, world, "tiny", flags, flags)
        assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] > 0
    c.set_material_map(5, -1, rt.MAP_OPACITY); c.commit()
    p = context(rt, [], world.tiny_plain)
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, p))) and c.stats().kernel_launches[rt.K_BOUNCE] > 0
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 6. invariance
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_invariance(rt, world):
    p = context(rt, [], world.plain)
    base, base_cnt, lights = frame(rt, p), counts(p), p.lights()
    nmat = len(world.plain.materials)
    # an all-255 map on every material
    full = np.full((16, 16, 4), 255, np.uint8); full[..., :3] = 7
    sc = CutScene(world.plain, world.free_uvs, [(full, True)], [-1] * nmat, [0] * nmat)
    c = context(rt, [], sc)
    assert c.opacity(np.array([[1.0, 0.2, 0.3, 0.0]], np.float32))[0, 0] == 1.0
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and counts(c) == base_cnt
    c.close()
    # an all-0 map on the material only the second monkey's mesh uses == that instance hidden
    clear = np.zeros((4, 4, 4), np.uint8); clear[..., :3] = 200
    sc = CutScene(world.plain, world.free_uvs, [(clear, False)], [-1] * nmat, [(0 if m == GLASS2 else -1) for m in range(nmat)])
    c = context(rt, [], sc)
    img, cnt = frame(rt, c), counts(c)
    p.set_instance_visible(3, False); p.commit()
    assert np.array_equal(bits(img), bits(frame(rt, p))) and cnt == counts(p) and not np.array_equal(bits(img), bits(base))
    p.set_instance_visible(3, True); p.commit()
    c.close()
    # an opacity map on the emitter's material alone changes nothing
    sc = CutScene(world.plain, world.free_uvs, [(clear, False)], [-1] * nmat, [(0 if m == LAMP else -1) for m in range(nmat)])
    c = context(rt, [], sc)
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and counts(c) == base_cnt and np.array_equal(bits(c.lights()), bits(lights))
    assert c.stats().kernel_launches[rt.K_SHADE] > 0
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 7. commits
# ------------------------------------------------------------------------------------------------
def bind_opacity(rt, c, sc):
    for m, t in enumerate(sc.opacity_maps):
        c.set_material_map(m, t, rt.MAP_OPACITY)


@pytest.mark.gpu
def test_map_commits_leave_the_tree_alone(rt, world):
    c = context(rt, [], world.plain)
    base, tree, refits = frame(rt, c), c.tree_hash(), c.stats().bvh_refits
    bind(c, world.cut, maps=False); c.commit()                      # UVs and textures, no map
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and (c.tree_hash(), c.stats().bvh_refits) == (tree, refits)
    bind_opacity(rt, c, world.cut)
    with pytest.raises(rt.RtxError):
        c.render(rt.Params(**PT))                                   # edits need a commit
    c.commit()
    cut = frame(rt, c)
    assert (c.tree_hash(), c.stats().bvh_refits) == (tree, refits) and not np.array_equal(bits(cut), bits(base))
    assert np.array_equal(bits(cut), bits(world.expect("cut", 0)[0]))
    for m in range(len(world.plain.materials)):
        c.set_material_map(m, -1, rt.MAP_OPACITY)
    c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(base)) and (c.tree_hash(), c.stats().bvh_refits) == (tree, refits)
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["default", "gpu_build"])
def test_cutouts_stay_on_their_triangles_through_edits(rt, world, config):
    """a deform and a transform edit in one commit, then a hide, then a show: each image is the oracle's of the equivalent edited scene"""
    c = context(rt, CONFIGS[config], world.cut)
    c.update_mesh_vertices(MONKE, world.monke2)
    c.set_instance_transform(2, world.card_o2w2)
    c.commit()
    check_transport(rt, c, world, "edited1", 0, config)
    c.set_instance_visible(3, False); c.commit()
    check_transport(rt, c, world, "edited2", 0, config)
    c.set_instance_visible(3, True); c.commit()
    check_transport(rt, c, world, "edited1", 0, config)
    c.close()


# ------------------------------------------------------------------------------------------------
# 8. partners
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_adaptive_guides_and_layers(rt, world):
    """render_adaptive with threshold 0 == render; the denoiser's guides and debug layer 12 show, through a hole, the material behind it: those of the equivalent scene"""
    c = context(rt, [], world.cut)
    ref = frame(rt, c)
    c.clear(W, H)
    c.render_adaptive(rt.Params(**PT), 2, 2, PT["spp"], 0.0)
    assert np.array_equal(bits(c.read_accum()), bits(ref))
    e = context(rt, [], cut_equivalent(rt, world.cut))
    p = context(rt, [], world.plain)
    g = c.denoise_guides(W, H)
    assert np.array_equal(bits(g), bits(e.denoise_guides(W, H))) and not np.array_equal(bits(g), bits(p.denoise_guides(W, H)))
    for layer in (10, 11, 12, 13, 14, 15, 17):
        assert np.array_equal(c.read_layer(layer, W, H), e.read_layer(layer, W, H)), layer
    assert not np.array_equal(c.read_layer(12, W, H), p.read_layer(12, W, H))
    p.close(); e.close(); c.close()


@pytest.mark.gpu
def test_restir_and_pass1_ignore_cutouts(rt, orc, world):
    """render_restir and render_v6_pass1 on the cut-out scene == the oracle on the PLAIN scene"""
    c = context(rt, [], world.cut)
    o = orc.Oracle().load(world.plain, W / H)
    vp = world.plain.view_proj(W / H)
    c.set_camera(*vp); c.set_camera(*vp); o.set_camera(*vp); o.set_camera(*vp)      # previous view = current view
    p = rt.Params(width=W, height=H, spp=2, max_bounces=3, nee_samples=4, flags=0, frame_seed=3)
    c.restir_reset(); c.clear(W, H); c.render_restir(p)
    acc, st, cnt = o.restir_frames(p)
    assert counts(c) == cnt
    ld, lg, ls = c.read_restir_last()
    assert np.array_equal(ld, st[3]) and np.array_equal(lg, st[4]) and np.array_equal(ls, st[5])
    assert np.array_equal(bits(c.read_accum()), bits(acc))
    p1 = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=4, flags=0, frame_seed=5)
    c.clear(W, H); c.render_v6_pass1(p1)
    got, (gd, gg, gs) = c.read_accum(), c.read_pass1_buffers()
    _, (cd, cg, cs), cnt1 = o.render_v6_pass1(p1)
    assert counts(c) == cnt1 and np.array_equal(gd, cd) and np.array_equal(gg, cg) and np.array_equal(gs, cs)
    q = context(rt, [], world.plain)
    q.clear(W, H); q.render_v6_pass1(p1)
    assert np.array_equal(bits(q.read_accum()), bits(got))
    o.close(); q.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 9. errors and state
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_errors_leave_the_scene_committed(rt, world, tmp_path):
    c = context(rt, [], world.cut)
    ref = frame(rt, c)
    L = rt.lib
    nmat, ntex = len(world.plain.materials), len(world.cut.textures)
    for k, call in enumerate([lambda: L.rtx_set_material_map(c._h, 1, 1, 0), lambda: L.rtx_set_material_map(c._h, 1, 3, 0), lambda: L.rtx_set_material_map(c._h, 1, rt.MAP_OPACITY, ntex),
                              lambda: L.rtx_set_material_map(c._h, 1, rt.MAP_OPACITY, -2), lambda: L.rtx_set_material_map(c._h, nmat, rt.MAP_OPACITY, 0)]):
        assert call() == -1, k                                      # RTX_ERR_INVALID
        assert np.array_equal(bits(frame(rt, c)), bits(ref)), k     # ... untouched, and still committed
    with pytest.raises(rt.RtxError):
        c.set_material_map(1, 0, 3)
    hits = np.zeros((1, 4), np.float32); hits[0, 3:].view(np.uint32)[:] = c.stats().triangles
    assert L.rtx_debug_opacity(c._h, hits.ctypes.data_as(rt.C.c_void_p), 1, np.zeros(2, np.float32).ctypes.data_as(rt.C.c_void_p)) == -1
    with pytest.raises(rt.RtxError):
        c.save_scene_cache(tmp_path / "t.rtxscn")                   # the file holds no texels
    # rtx_set_materials replaces the table: no material has an opacity map afterwards, and the cache can be written again
    c.set_materials(world.plain.materials); c.commit()
    p = context(rt, [], world.plain)
    assert np.array_equal(bits(frame(rt, c)), bits(frame(rt, p)))
    c.save_scene_cache(tmp_path / "t.rtxscn")
    p.close(); c.close()


# ------------------------------------------------------------------------------------------------
# 10. the command line
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_renders_map_d(rt, tmp_path):
    """rtx_render on an OBJ whose MTL names a PGM map_d: differs from --no-cutouts, equals the Python path's image; --no-cutouts and --no-textures are the plain scene"""
    from test_cutout_ref import leaf_mask, write_card
    from test_denoise import read_exr_rgb
    mask = leaf_mask(np.random.default_rng(5))
    (tmp_path / "mask.pgm").write_bytes(b"P5 16 16 255\n" + mask.tobytes())
    files, mtl = write_card(tmp_path, "map_d mask.pgm\n")
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
    base = [exe, "--obj", files[0], "--mtl", str(tmp_path), "--w", str(W), "--h", str(H), "--spp", "4", "--gpus", "1"]

    def cli(name, *extra):
        out = str(tmp_path / name)
        r = subprocess.run(base + ["--out", out] + list(extra), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-1000:])
        return read_exr_rgb(out)

    sc = rt.Scene.from_obj(files, mtl)
    assert sc.opacity_maps == [-1, -1, 0, -1]
    p = rt.Params(width=W, height=H, spp=4, sample_base=1, max_bounces=8, nee_samples=1, rr_start=3, frame_seed=1, flags=0)

    def python(scene):
        c = rt.Context(0)
        c.upload(scene, W / H); c.clear(W, H); c.render(p)
        a = c.read_accum(); c.close()
        return a[..., :3] / np.maximum(a[..., 3:], np.float32(1.0))

    cut = python(sc)
    sc.opacity_maps = []
    plain = python(sc)
    assert not np.array_equal(bits(cut), bits(plain)) and cut.sum() > 0
    assert np.array_equal(bits(cli("c.exr")), bits(cut))
    assert np.array_equal(bits(cli("n.exr", "--no-cutouts")), bits(plain))
    assert np.array_equal(bits(cli("t.exr", "--no-textures")), bits(plain))

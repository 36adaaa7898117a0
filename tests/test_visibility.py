"""Instance visibility: rtx_set_instance_visible + rtx_commit_scene hide or show an instance by a refit-only commit (k_refit_tris writes never-hit triangle records,
k_refit_nodes leaves them out of every box), ids stay.  Every check is bit-exact against a FRESH oracle loaded with the hidden instances REMOVED (the oracle has no
visibility; when a removed instance is not the last one, its triangle and instance ids are mapped back to the original numbering) and against a fresh context built
without them."""
import os
import subprocess

import numpy as np
import pytest

from test_deform import ArrayScene, bits, place, random_rays, sine_deform

W, H = 96, 54
PT = dict(width=W, height=H, spp=4, max_bounces=3, nee_samples=1, flags=0)      # GGX + NEE
ATRIUM, GRID, MONKE = 0, 1, 2                                                    # meshes
MISS = np.uint32(0xFFFFFFFF)
T4 = place(0.8, 0.5, 0.2, -0.45, 0.3, 0.35)                                      # instance 4 as built: mirrored, non-uniformly scaled
T4_MOVED = place(0.55, 0.62, -0.1, -0.4, 0.33, 0.3)
T5 = place(1.2, 0.9, 0.4, 1, 1, 1)                                               # the extra grid of the rebuild test


def make_scene(rt, golden_dir):
    """0: a ~6000-triangle atrium with its own lights (the whole scene stays above the GPU builder's 4096-triangle threshold); 1, 2: one emissive 6 x 6-quad grid
    instanced twice, the second shifted by half a cell so that the two interleave (hidden and visible triangles share leaf slots); 3: monke.obj; 4: monke.obj mirrored and
    non-uniformly scaled, large enough to own whole subtrees"""
    big = rt.Scene.sponza_class(6000, 260)
    small = rt.Scene.from_obj([os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    nm = len(big.materials)
    lamp = np.array(big.materials[np.argmax(big.materials[:, 8:11].sum(1))], np.float32, copy=True)
    lamp[8:11] = (6.0, 5.0, 4.0)
    materials = np.concatenate([np.asarray(big.materials, np.float32), np.asarray(small.materials, np.float32), lamp[None]])
    assert len(big.meshes) == 1 and len(big.instances) == 1
    meshes = list(big.meshes)
    base = sum(len(m) for _, _, m in big.meshes)
    g = 7
    gx, gz = np.meshgrid(np.linspace(-0.15, 0.15, g), np.linspace(-0.15, 0.15, g), indexing="ij")
    lv = np.zeros((g * g, 7), np.float32); lv[:, 0], lv[:, 1], lv[:, 2], lv[:, 6] = gx.ravel(), 0.0, gz.ravel(), float(base)
    li = []
    for a in range(g - 1):
        for b in range(g - 1):
            q = a * g + b
            li += [q, q + g, q + 1, q + 1, q + g, q + g + 1]
    li = np.array(li, np.uint32)
    meshes.append((lv, li, np.full(len(li), nm + len(small.materials), np.uint32))); base += len(li)
    v, i, m = small.meshes[0]
    v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)
    meshes.append((v, i, np.asarray(m, np.uint32) + np.uint32(nm)))
    instances = list(big.instances) + [(GRID, place(-0.6, 1.1, 0.0, 1, 1, 1)), (GRID, place(-0.575, 1.1, 0.025, 1, 1, 1)),
                                       (MONKE, place(0.0, 0.3, 0.0, 0.25, 0.25, 0.25)), (MONKE, T4)]
    return ArrayScene(materials, meshes, instances, big.view_proj, -1.5, 1.5), big


def without(sc, hidden):
    """the scene with the instances in `hidden` REMOVED (every mesh stays: the material-id bases do not move), and the maps from its numbering back to the original one:
    tri_map[removed-scene triangle id] = original id, inst_map[removed-scene instance id] = original id"""
    ntri = [len(sc.meshes[mesh][1]) // 3 for mesh, _ in sc.instances]
    base = np.concatenate([[0], np.cumsum(ntri)]).astype(np.int64)
    keep = [k for k in range(len(sc.instances)) if k not in hidden]
    tri_map = np.concatenate([np.arange(base[k], base[k + 1]) for k in keep] + [np.zeros(0, np.int64)]).astype(np.uint32)
    r = ArrayScene(sc.materials, sc.meshes, [sc.instances[k] for k in keep], sc._vp, sc.lo, sc.hi)
    return r, tri_map, np.array(keep, np.uint32)


def with_instance(sc, inst, o2w):
    s = ArrayScene(sc.materials, sc.meshes, sc.instances, sc._vp, sc.lo, sc.hi)
    s.instances[inst] = (s.instances[inst][0], o2w)
    return s


class World:
    """the scene of this module, built once, and what the oracle / a fresh context say about a (scene, hidden set) state: computed once, shared by the configurations"""
    def __init__(self, rt, orc, golden_dir):
        self.rt, self.orc = rt, orc
        self.full, self._keep = make_scene(rt, golden_dir)
        self.moved = with_instance(self.full, 4, T4_MOVED)
        mv, mi, _ = self.full.meshes[MONKE]
        self.monke2 = sine_deform(mv, mi, 0.06, 9.0, 0.0)
        self.deformed = self.full.with_meshes([(MONKE, self.monke2)])
        self.grown = ArrayScene(self.full.materials, self.full.meshes, self.full.instances + [(GRID, T5)], self.full._vp, self.full.lo, self.full.hi)
        self.variants = dict(full=self.full, moved=self.moved, deformed=self.deformed, grown=self.grown)
        self.rays = None
        self.states = {}

    def expect(self, variant, hidden):
        key = (variant, frozenset(hidden))
        if key in self.states:
            return self.states[key]
        rt = self.rt
        sc, tri_map, inst_map = without(self.variants[variant], key[1])
        o = self.orc.Oracle().load(sc, W / H)
        if self.rays is None:                                # camera rays + 20 000 random ones: one query set for every state (the camera never moves)
            self.rays = np.concatenate([o.primary_rays(rt.Params(width=W, height=H)), random_rays(20000, 91, self.full.lo, self.full.hi)])
        closest = o.trace_closest(self.rays, 1)
        prim = closest[:, 3].view(np.uint32)                 # (a view: the id column is rewritten in place, in the original numbering)
        hit = prim != MISS
        prim[hit] = tri_map[prim[hit]]
        lights = o.lights()
        if len(lights):
            lights[:, 7].view(np.uint32)[:] = inst_map[lights[:, 7].view(np.uint32)]
        acc, cnt = o.render(rt.Params(**PT))
        e = dict(rays=self.rays, closest=closest, any=o.trace_any(self.rays, 1), lights=lights, accum=acc, counts=cnt)
        o.close()
        f = rt.Context(0); f.upload(sc, W / H); f.clear(W, H); f.render(rt.Params(**PT)); e["fresh"] = f.read_accum(); f.close()
        self.states[key] = e
        return e


@pytest.fixture(scope="module")
def world(rt, orc, golden_dir):
    return World(rt, orc, golden_dir)


def check(rt, c, e, tag):
    assert c.validate_bvh() == 0, tag
    assert np.array_equal(bits(c.trace_closest(e["rays"])), bits(e["closest"])), tag
    assert np.array_equal(c.trace_any(e["rays"]), e["any"]), tag
    assert np.array_equal(bits(c.lights()), bits(e["lights"])), tag
    assert c.stats().lights == len(e["lights"]), tag
    c.clear(W, H); c.render(rt.Params(**PT))
    img, st = c.read_accum(), c.stats()
    assert np.array_equal(bits(img), bits(e["accum"])), tag
    assert (st.rays_primary, st.rays_extension, st.rays_shadow) == e["counts"], tag
    assert np.array_equal(bits(img), bits(e["fresh"])), tag
    return img


def context(rt, opts, scene):
    c = rt.Context(0)
    for o, v in opts:
        c.set_option(getattr(rt, o), v)
    c.upload(scene, W / H)
    return c


def flip(c, hide=(), show=()):
    for k in hide:
        c.set_instance_visible(k, False)
    for k in show:
        c.set_instance_visible(k, True)


CONFIGS = {"default": [], "gpu_build": [("OPT_GPU_BUILD", 1)], "host_refit": [("OPT_GPU_REFIT", 0)], "full_refit": [("OPT_PARTIAL_REFIT", 0)]}
TREE_CONFIGS = ["default", "gpu_build"]


# ------------------------------------------------------------------------------------------------
# CPU
# ------------------------------------------------------------------------------------------------
def test_visibility_entry_points_are_bound(rt):
    """the C-ABI and host-layer entry points exist in the library and the Python layer wraps them (no GPU)"""
    assert rt.lib.rtx_set_instance_visible and rt.lib.rtxh_renderer_set_instance_visible
    assert callable(rt.Context.set_instance_visible) and callable(rt.Renderer.set_instance_visible)
    assert rt.lib.rtx_set_instance_visible(None, 0, 0) == -1             # no context: RTX_ERR_INVALID, nothing touched


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_sequence_of_hides_and_shows(rt, world, config):
    """as built; hide 4; also hide 2 (mixed leaves, lights dropped); show 4 while moving it in the same commit; hide 3 (a middle instance: the id mapping); show everything
    (and 4 back where it was built, so that the image is the as-built one).  After every commit: the tree validates, closest / any hits, the light records, the image
    and its ray counts equal the oracle's for the scene with the hidden instances removed, the image equals a fresh context's — and the commit was a refit.
    default: host-built tree, partial GPU refit; gpu_build: device-built tree; host_refit: RTX_OPT_GPU_REFIT 0; full_refit: RTX_OPT_PARTIAL_REFIT 0."""
    c = context(rt, CONFIGS[config], world.full)
    first = check(rt, c, world.expect("full", ()), (config, "as built"))
    total = c.stats().triangles
    steps = [("hide 4", lambda: flip(c, hide=[4]), "full", (4,)),
             ("hide 2", lambda: flip(c, hide=[2]), "full", (2, 4)),
             ("show 4, moved", lambda: (flip(c, show=[4]), c.set_instance_transform(4, T4_MOVED)), "moved", (2,)),
             ("hide 3", lambda: flip(c, hide=[3]), "moved", (2, 3)),
             ("show all", lambda: (flip(c, show=[2, 3]), c.set_instance_transform(4, T4)), "full", ())]
    img = None
    for k, (tag, act, variant, hidden) in enumerate(steps):
        act(); c.commit()
        st = c.stats()
        assert st.bvh_refits == k + 1 and st.triangles == total, (config, tag, st.bvh_refits)
        img = check(rt, c, world.expect(variant, hidden), (config, tag))
    assert np.array_equal(bits(img), bits(first)), config
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", TREE_CONFIGS)
def test_hide_then_show_restores_the_tree(rt, world, config):
    """transform-only commit (GPU-refitted boxes on both sides of the comparison) -> hash; hide 4; show 4: the device tree is what it was, node and triangle records"""
    c = context(rt, CONFIGS[config], world.full)
    c.set_instance_transform(4, T4_MOVED); c.commit()
    h0 = c.tree_hash()
    flip(c, hide=[4]); c.commit()
    assert c.tree_hash() != h0
    flip(c, show=[4]); c.commit()
    assert c.tree_hash() == h0 and c.stats().bvh_refits == 3
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", TREE_CONFIGS)
def test_everything_hidden(rt, world, config):
    """every instance hidden: a black image with counts (W H spp, 0, 0), no lights, every closest hit a miss, every any hit 0, a finite and reproducible tree cost; then
    everything shown again is the scene as built"""
    e0 = world.expect("full", ())
    c = context(rt, CONFIGS[config], world.full)
    flip(c, hide=range(5)); c.commit()
    assert c.validate_bvh() == 0
    p = rt.Params(**PT)
    c.clear(W, H); c.render(p)
    st = c.stats()
    assert (st.rays_primary, st.rays_extension, st.rays_shadow) == (W * H * p.spp, 0, 0) and st.lights == 0 and st.bvh_refits == 1
    assert not c.read_accum()[..., :3].any()
    assert c.lights().shape == (0, 20)
    assert (c.trace_closest(e0["rays"])[:, 3].view(np.uint32) == MISS).all() and not c.trace_any(e0["rays"]).any()
    cost = c.tree_cost()
    assert np.isfinite(cost).all() and cost == c.tree_cost()
    flip(c, show=range(5)); c.commit()
    check(rt, c, e0, (config, "all shown again"))
    c.close()


@pytest.mark.gpu
def test_hidden_and_deformed(rt, world):
    """hide 3, new vertices for monke, one commit: the state is 'without 3' while the visible instance 4 shows the new vertices; showing 3 then shows them in both places"""
    c = context(rt, [], world.full)
    flip(c, hide=[3]); c.update_mesh_vertices(MONKE, world.monke2); c.commit()
    assert c.stats().bvh_refits == 1
    check(rt, c, world.expect("deformed", (3,)), "hidden and deformed")
    flip(c, show=[3]); c.commit()
    assert c.stats().bvh_refits == 2
    check(rt, c, world.expect("deformed", ()), "shown after the deformation")
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", TREE_CONFIGS)
def test_rebuild_keeps_visibility(rt, world, config):
    """hide 4, then rtx_add_instance of another grid: the commit rebuilds (no refit counted) and instance 4 stays hidden, boxes and lights included"""
    c = context(rt, CONFIGS[config], world.full)
    flip(c, hide=[4]); c.commit()
    assert c.add_instance(GRID, T5) == 5
    c.commit()
    assert c.stats().bvh_refits == 0
    check(rt, c, world.expect("grown", (4,)), (config, "rebuilt with 4 hidden"))
    c.close()


@pytest.mark.gpu
def test_tiny_scene(rt, orc):
    """Cornell Box + a 12-triangle box instance (44 triangles, the tiny-scene path): with the box hidden rtx_render and one ReSTIR frame equal the oracle's plain Cornell
    Box, with it shown again the oracle's scene with the box"""
    cb = rt.Scene.cornell()
    base = sum(len(m) for _, _, m in cb.meshes)
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    bv = np.zeros((8, 7), np.float32); bv[:, :3] = corners; bv[:, 6] = float(base)
    bi = np.array([0, 1, 3, 0, 3, 2, 4, 6, 7, 4, 7, 5, 0, 4, 5, 0, 5, 1, 2, 3, 7, 2, 7, 6, 0, 2, 6, 0, 6, 4, 1, 5, 7, 1, 7, 3], np.uint32)
    mats = np.asarray(cb.materials, np.float32)
    meshes = list(cb.meshes) + [(bv, bi, np.full(len(bi), int(np.argmin(mats[:, 8:11].sum(1))), np.uint32))]      # (a material that does not emit)
    insts = list(cb.instances) + [(1, place(0.42, 0.31, 0.37, 0.2, 0.25, 0.2))]
    full = ArrayScene(mats, meshes, insts, cb.view_proj, -0.2, 1.2)
    plain = ArrayScene(mats, meshes, insts[:1], cb.view_proj, -0.2, 1.2)
    pt = rt.Params(**PT)
    rs = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=4, flags=0, frame_seed=5)
    c = rt.Context(0); c.upload(full, W / H)
    assert c.stats().triangles == 44
    for tag, sc, visible, refits in (("box hidden", plain, False, 1), ("box shown", full, True, 2)):
        c.set_instance_visible(1, visible); c.commit()
        assert c.stats().bvh_refits == refits and c.stats().triangles == 44, tag
        assert c.validate_bvh() == 0, tag
        o = orc.Oracle().load(sc, W / H)
        acc, cnt = o.render(pt)
        c.clear(W, H); c.render(pt)
        s = c.stats()
        assert np.array_equal(bits(c.read_accum()), bits(acc)), tag
        assert (s.rays_primary, s.rays_extension, s.rays_shadow) == cnt, tag
        vp = sc.view_proj(W / H)
        c.set_camera(*vp); c.set_camera(*vp); o.set_camera(*vp); o.set_camera(*vp)      # previous view = current view
        c.restir_reset(); c.clear(W, H); c.render_restir(rs)
        acc, st, cnt = o.restir_frames(rs)
        s = c.stats()
        assert (s.rays_primary, s.rays_extension, s.rays_shadow) == cnt, tag
        ld, lg, ls = c.read_restir_last()
        assert np.array_equal(ld, st[3]) and np.array_equal(lg, st[4]) and np.array_equal(ls, st[5]), tag
        assert np.array_equal(bits(c.read_accum()), bits(acc)), tag
        o.close()
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", TREE_CONFIGS)
def test_rays_do_not_pay_for_hidden_triangles(rt, world, config):
    """rays aimed at monke 4 whose closest hit lies on it (at least 200): with 4 hidden they test strictly fewer triangles; over the whole query set the summed node steps
    and the summed triangle tests are each no more than with 4 shown"""
    e0 = world.expect("full", ())
    sc = world.full
    ntri = [len(sc.meshes[mesh][1]) // 3 for mesh, _ in sc.instances]
    lo4, hi4 = sum(ntri[:4]), sum(ntri[:5])
    v = np.asarray(sc.meshes[MONKE][0], np.float32).reshape(-1, 7)[:, :3]
    m = np.asarray(T4, np.float32).reshape(4, 4)
    wv = v @ m[:3, :3] + m[3, :3]                                        # (row-vector convention: element (row r, col c) of the column-vector matrix at m[c * 4 + r])
    rng = np.random.default_rng(17)
    n = 2000
    org = rng.uniform(sc.lo, sc.hi, (n, 3)); org[:, 1] = np.abs(org[:, 1]) * 0.9 + 0.05; org[:, 2] *= 0.5
    d = wv[rng.integers(0, len(wv), n)] - org
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    aimed = np.zeros((n, 8), np.float32); aimed[:, 0:3], aimed[:, 3], aimed[:, 4:7], aimed[:, 7] = org, 1e-4, d, 1e4
    c = context(rt, CONFIGS[config], sc)
    prim = c.trace_closest(aimed)[:, 3].view(np.uint32)
    kept = aimed[(prim >= lo4) & (prim < hi4)]
    assert len(kept) >= 200, len(kept)
    shown_all, shown_kept = c.trace_stats(e0["rays"]), c.trace_stats(kept)
    flip(c, hide=[4]); c.commit()
    hidden_all, hidden_kept = c.trace_stats(e0["rays"]), c.trace_stats(kept)
    sums = [float(a[:, k].astype(np.float64).sum()) for a in (shown_all, hidden_all, shown_kept, hidden_kept) for k in (1, 2)]
    print(config, "node steps / triangle tests: all rays shown", sums[0:2], "hidden", sums[2:4], "| kept rays shown", sums[4:6], "hidden", sums[6:8])
    assert sums[2] <= sums[0] and sums[3] <= sums[1], sums
    assert sums[7] < sums[5], sums
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("wavefront", [1, 0])
def test_restir_frame_after_a_hide(rt, orc, world, wavefront):
    """two frames, hide 4 (the last instance: objIDs need no mapping), rtx_restir_reset, one frame: the image, the three history buffers and the counts equal the oracle's
    first frame of the scene without 4 (a visibility change leaves the history alone; a caller who wants no ghosting resets it)"""
    c = context(rt, [("OPT_RESTIR_WAVEFRONT", wavefront)], world.full)
    p = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=4, flags=0, frame_seed=5)
    c.restir_reset(); c.clear(W, H); c.render_restir(rt.Params(width=W, height=H, spp=2, max_bounces=3, nee_samples=4, flags=0, frame_seed=3))
    flip(c, hide=[4]); c.commit()
    sc1, _, _ = without(world.full, {4})
    vp = sc1.view_proj(W / H)
    o = orc.Oracle().load(sc1, W / H)
    c.set_camera(*vp); c.set_camera(*vp); o.set_camera(*vp); o.set_camera(*vp)      # previous view = current view
    c.restir_reset(); c.clear(W, H); c.render_restir(p)
    acc, st, cnt = o.restir_frames(p)
    s = c.stats()
    assert (s.rays_primary, s.rays_extension, s.rays_shadow) == cnt
    ld, lg, ls = c.read_restir_last()
    assert np.array_equal(ld, st[3]) and np.array_equal(lg, st[4]) and np.array_equal(ls, st[5])
    assert np.array_equal(bits(c.read_accum()), bits(acc))
    c.close(); o.close()


@pytest.mark.gpu
def test_errors_and_state(rt, world, tmp_path):
    """an unknown instance is RTX_ERR_INVALID and the next render equals the previous one; a change needs a commit (a render in between is RTX_ERR_STATE); the value an
    instance already has dirties nothing; rtx_save_scene_cache refuses while an instance is hidden, writes no file, and round-trips once everything is shown"""
    e0 = world.expect("full", ())
    c = context(rt, [], world.full)
    p = rt.Params(**PT)
    c.clear(W, H); c.render(p); first = c.read_accum()
    with pytest.raises(rt.RtxError) as ei:
        c.set_instance_visible(5, False)
    assert "(-1)" in str(ei.value) and "set_instance_visible" in str(ei.value)
    c.clear(W, H); c.render(p)
    assert np.array_equal(bits(c.read_accum()), bits(first)) and np.array_equal(bits(first), bits(e0["accum"]))
    c.set_instance_visible(3, True)                                   # already visible: nothing to commit
    c.clear(W, H); c.render(p)
    assert np.array_equal(bits(c.read_accum()), bits(first)) and c.stats().bvh_refits == 0
    c.set_instance_visible(4, False)
    with pytest.raises(rt.RtxError) as ei:
        c.render(p)
    assert "(-4)" in str(ei.value)
    c.commit()
    assert c.stats().bvh_refits == 1
    c.set_instance_visible(4, False)                                  # already hidden
    c.clear(W, H); c.render(p)
    assert np.array_equal(bits(c.read_accum()), bits(world.expect("full", (4,))["accum"])) and c.stats().bvh_refits == 1
    path = tmp_path / "hidden.rtxc"
    with pytest.raises(rt.RtxError) as ei:
        c.save_scene_cache(path)
    assert "(-4)" in str(ei.value) and not path.exists()
    c.set_instance_visible(4, True); c.commit()
    c.save_scene_cache(path)
    c.close()
    d = rt.Context(0); d.load_scene_cache(path); d.set_camera(*world.full.view_proj(W / H))
    check(rt, d, e0, "loaded cache")
    d.close()


@pytest.mark.gpu
def test_visibility_from_the_cpp_host(rt, orc, golden_dir, tmp_path):
    """(a) Renderer::SetInstanceVisible + OnUpdate + OnRender through the facade's C entry points: two accumulated path-traced frames on garage.obj + monke.obj, the monkey
    hidden in the first and shown in the second, equal the oracle's.  (b) `rtx_render --hide 1`: the facade, one native rank and two native ranks
    (MultiGpuFrame::SetInstanceVisible: EVERY rank commits) write byte-identical images, which differ from the image with nothing hidden."""
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    Wf, Hf = 96, 56
    arr = ArrayScene(np.asarray(sc.materials, np.float32), sc.meshes, sc.instances, sc.view_proj, -1.0, 1.0)
    r = rt.Renderer(Wf, Hf, "visibility", 0)
    r.set_scene(sc); r.on_init()
    r.params.max_bounces = 3
    acc_o = np.zeros((Hf, Wf, 4), np.float32)
    for k, hidden in enumerate(({1}, set())):
        r.set_instance_visible(1, not hidden)
        r.on_update(); r.on_render()
        o = orc.Oracle().load(without(arr, hidden)[0], Wf / Hf)
        acc_o, _ = o.render(rt.Params(width=Wf, height=Hf, spp=1, sample_base=1, max_bounces=3, nee_samples=1, rr_start=3, frame_seed=k + 1, flags=0), acc_o)
        o.close()
    assert np.array_equal(bits(r.read_accum()), bits(acc_o))
    with pytest.raises(rt.RtxError):
        r.set_instance_visible(2, False)
    r.close()
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "royaltracer-dx_amd", "rtx_render")
    sargs = ["--obj", os.path.join(golden_dir, "garage.obj") + "," + os.path.join(golden_dir, "monke.obj"), "--mtl", golden_dir + "/", "--spp", "2", "--bounces", "4", "--w", "192", "--h", "108", "--gather", "copy"]
    blobs = {}
    for tag, extra in (("plain", []), ("facade", ["--hide", "1"]), ("n1", ["--hide", "1", "--gpus", "1", "--devices", "0"]), ("n2", ["--hide", "1", "--gpus", "2", "--devices", "0,0"])):
        out = tmp_path / f"hide_{tag}.exr"
        cmd = [exe] + sargs + ["--out", str(out)] + extra
        q = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert q.returncode == 0, (cmd, q.stderr[-2000:])
        blobs[tag] = out.read_bytes()
    assert blobs["n1"] == blobs["facade"] and blobs["n2"] == blobs["facade"] and blobs["plain"] != blobs["facade"]

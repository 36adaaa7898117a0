"""Deforming meshes: rtx_update_mesh_vertices + rtx_commit_scene re-derive the triangles of the changed meshes' instances and refit the resident tree (k_reflatten,
k_refit_tris / k_refit_nodes), RTX_OPT_DEFORM_REBUILD chooses between refit and rebuild by the tree's visit cost (k_tree_cost).  Every check is bit-exact: against a FRESH
oracle loaded with the deformed arrays (the oracle has no vertex update; it rebuilds) or against a fresh context committed from scratch."""
import ctypes as C
import os

import numpy as np
import pytest

W, H = 96, 54


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def random_rays(n, seed, lo, hi, tmax=1e4):
    rng = np.random.default_rng(seed)
    o = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
    d = rng.normal(size=(n, 3)).astype(np.float32)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 1e-4, d.astype(np.float32), tmax
    return r


def vertex_normals(pos, idx):
    """area-weighted vertex normals (n, 3) float64; a vertex no triangle with area touches gets (0, 0, 0) = 'use the flat normal' (Hit_v6.hlsl:40-46)"""
    tri = np.asarray(idx, np.int64).reshape(-1, 3)
    p = np.asarray(pos, np.float64)
    fn = np.cross(p[tri[:, 1]] - p[tri[:, 0]], p[tri[:, 2]] - p[tri[:, 0]])
    n = np.zeros_like(p)
    for k in range(3):
        np.add.at(n, tri[:, k], fn)
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.maximum(ln, 1e-300), 0.0)


def sine_deform(verts, idx, amp, freq, phase):
    """a sine displacement along the vertex normal; the normals are then re-derived from the displaced surface.  Column 6 (Vertex.normal.w) is kept"""
    v = np.array(verts, np.float32, copy=True).reshape(-1, 7)
    n = vertex_normals(v[:, :3], idx)
    d = amp * np.sin(freq * (v[:, 0].astype(np.float64) + 2.0 * v[:, 1] + 3.0 * v[:, 2]) + phase)
    v[:, :3] = (v[:, :3].astype(np.float64) + d[:, None] * n).astype(np.float32)
    v[:, 3:6] = vertex_normals(v[:, :3], idx).astype(np.float32)
    return v


def scramble(verts, idx, seed):
    """every vertex displaced by a pseudo-random vector of the object's own extent: a refit keeps the topology, so nearly every box below the object's root grows to cover it"""
    v = np.array(verts, np.float32, copy=True).reshape(-1, 7)
    ext = v[:, :3].max(0) - v[:, :3].min(0)
    v[:, :3] += ((np.random.default_rng(seed).random((len(v), 3)) - 0.5) * ext).astype(np.float32)
    v[:, 3:6] = vertex_normals(v[:, :3], idx).astype(np.float32)
    return v


class ArrayScene:
    """meshes / materials / instances as arrays (duck-typed like rt.Scene for Context.upload and Oracle.load); meshes are replaced, never edited in place"""
    def __init__(self, materials, meshes, instances, view_proj, lo, hi):
        self.materials, self.meshes, self.instances, self._vp, self.lo, self.hi = materials, list(meshes), list(instances), view_proj, lo, hi

    def view_proj(self, aspect):
        return self._vp(aspect)

    def with_meshes(self, updates):
        s = ArrayScene(self.materials, self.meshes, self.instances, self._vp, self.lo, self.hi)
        for mesh, v in updates:
            s.meshes[mesh] = (v, s.meshes[mesh][1], s.meshes[mesh][2])
        return s


def place(x, y, z, sx, sy, sz):
    m = np.eye(4, dtype=np.float32)
    m[0, 0], m[1, 1], m[2, 2] = sx, sy, sz
    m[3, 0], m[3, 1], m[3, 2] = x, y, z
    return m.reshape(16)


ATRIUM, MONKE, LAMP = 0, 1, 2


def make_atrium(rt, golden_dir):
    """a ~60 k-triangle atrium (one mesh, it carries the scene's two light triangles), monke.obj instanced twice — once mirrored and non-uniformly scaled — and a small
    emissive grid of its own (a mesh that emits and is not the atrium)"""
    big = rt.Scene.sponza_class(60000, 260)
    small = rt.Scene.from_obj([os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    nm = len(big.materials)
    lamp_mat = np.array(big.materials[np.argmax(big.materials[:, 8:11].sum(1))], np.float32, copy=True)
    lamp_mat[8:11] = (6.0, 5.0, 4.0)
    materials = np.concatenate([np.asarray(big.materials, np.float32), np.asarray(small.materials, np.float32), lamp_mat[None]])
    meshes = list(big.meshes)
    base = sum(len(m) for _, _, m in big.meshes)
    v, i, m = small.meshes[0]
    v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)          # Vertex.normal.w = the mesh's base in the scene's materialIDs
    meshes.append((v, i, np.asarray(m, np.uint32) + np.uint32(nm))); base += len(m)
    g = 7                                                                                  # 6 x 6 quads facing down
    gx, gz = np.meshgrid(np.linspace(-0.15, 0.15, g), np.linspace(-0.15, 0.15, g), indexing="ij")
    lv = np.zeros((g * g, 7), np.float32); lv[:, 0], lv[:, 1], lv[:, 2], lv[:, 6] = gx.ravel() - 0.6, 1.1, gz.ravel(), float(base)
    li = []
    for a in range(g - 1):
        for b in range(g - 1):
            q = a * g + b
            li += [q, q + g, q + 1, q + 1, q + g, q + g + 1]
    li = np.array(li, np.uint32)
    meshes.append((lv, li, np.full(len(li), nm + len(small.materials), np.uint32)))
    instances = list(big.instances) + [(MONKE, place(0.0, 0.3, 0.0, 0.25, 0.25, 0.25)), (MONKE, place(0.8, 0.45, 0.2, -0.3, 0.2, 0.25)), (LAMP, place(0, 0, 0, 1, 1, 1))]
    return ArrayScene(materials, meshes, instances, big.view_proj, -1.5, 1.5), big        # (big: keeps the native scene — and its camera — alive)


def atrium_steps(sc):
    """four successive deformations of monke; step 1 also bends the lamp (an emissive mesh), step 2 the atrium itself (which carries light triangles too)"""
    mv, mi, _ = sc.meshes[MONKE]; lv, li, _ = sc.meshes[LAMP]; av, ai, _ = sc.meshes[ATRIUM]
    out = []
    for k in range(4):
        mv = sine_deform(mv, mi, 0.06, 9.0 + k, 0.7 * k)
        up = [(MONKE, mv)]
        if k == 1:
            up.append((LAMP, sine_deform(lv, li, 0.04, 25.0, 0.3)))
        if k == 2:
            up.append((ATRIUM, sine_deform(av, ai, 0.01, 6.0, 0.2)))
        out.append(up)
    return out


def cornell_steps(sc):
    v, i, _ = sc.meshes[0]
    out = []
    for k in range(4):
        v = sine_deform(v, i, 0.03, 5.0 + k, 0.5 * k)
        out.append([(0, v)])
    return out


PT = dict(width=W, height=H, spp=4, max_bounces=3, nee_samples=1, flags=0)      # GGX + NEE


class World:
    """the scenes of this module, built once, and what the oracle / a fresh context say about each deformed state (computed once per state, shared by the configurations)"""
    def __init__(self, rt, orc, golden_dir):
        self.rt, self.orc = rt, orc
        self.atrium, self._keep = make_atrium(rt, golden_dir)
        c = rt.Scene.cornell()
        self.cornell = ArrayScene(np.asarray(c.materials, np.float32), c.meshes, c.instances, c.view_proj, -0.2, 1.2); self._keep2 = c
        self.states = {}
        self.steps = {"atrium": atrium_steps(self.atrium), "cornell": cornell_steps(self.cornell)}

    def scene(self, name, upto):
        """the scene after steps [0, upto)"""
        s = self.atrium if name == "atrium" else self.cornell
        for up in self.steps[name][:upto]:
            s = s.with_meshes(up)
        return s

    def expect(self, name, upto):
        key = (name, upto)
        if key not in self.states:
            self.states[key] = self.expect_scene(self.scene(name, upto), 90 + upto)
        return self.states[key]

    def expect_scene(self, sc, seed):
        rt, o = self.rt, self.orc.Oracle().load(sc, W / H)
        rays = np.concatenate([o.primary_rays(rt.Params(width=W, height=H)), random_rays(20000, seed, sc.lo, sc.hi)])
        acc, cnt = o.render(rt.Params(**PT))
        e = dict(rays=rays, closest=o.trace_closest(rays, 1), any=o.trace_any(rays, 1), lights=o.lights(), accum=acc, counts=cnt)
        o.close()
        f = rt.Context(0); f.upload(sc, W / H); f.clear(W, H); f.render(rt.Params(**PT)); e["fresh"] = f.read_accum(); f.close()
        return e


@pytest.fixture(scope="module")
def world(rt, orc, golden_dir):
    return World(rt, orc, golden_dir)


def check_state(rt, c, e, tag):
    assert c.validate_bvh() == 0, tag
    assert np.array_equal(bits(c.trace_closest(e["rays"])), bits(e["closest"])), tag
    assert np.array_equal(c.trace_any(e["rays"]), e["any"]), tag
    assert np.array_equal(bits(c.lights()), bits(e["lights"])), tag
    c.clear(W, H); c.render(rt.Params(**PT))
    img, st = c.read_accum(), c.stats()
    assert np.array_equal(bits(img), bits(e["accum"])), tag
    assert (st.rays_primary, st.rays_extension, st.rays_shadow) == e["counts"], tag
    assert np.array_equal(bits(img), bits(e["fresh"])), tag
    return img


# ------------------------------------------------------------------------------------------------
# CPU: the scene-level call (no GPU)
# ------------------------------------------------------------------------------------------------
def read_mesh(rt, scene, i):
    v, idx, mid, nv, ni = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint32(), C.c_uint32()
    assert rt.lib.rtxh_scene_mesh(scene._h, i, C.byref(v), C.byref(nv), C.byref(idx), C.byref(ni), C.byref(mid)) == 0
    return np.array((C.c_float * (nv.value * 7)).from_address(v.value), dtype=np.float32).reshape(-1, 7)


def test_scene_set_mesh_vertices_replaces_what_the_scene_reads_back(rt):
    """rtxh_scene_set_mesh_vertices (no GPU): the handle hands back the new vertices, Scene.set_mesh_vertices keeps its numpy copy in step, indices and material ids stay"""
    s = rt.Scene.cornell()
    v0, i0, m0 = s.meshes[0]
    v1 = sine_deform(v0, i0, 0.03, 5.0, 0.5)
    assert not np.array_equal(bits(v1[:, :6]), bits(v0[:, :6]))
    s.set_mesh_vertices(0, v1)
    assert np.array_equal(bits(read_mesh(rt, s, 0)), bits(v1))
    assert np.array_equal(bits(s.meshes[0][0]), bits(v1)) and s.meshes[0][1] is i0 and s.meshes[0][2] is m0
    assert s.num_triangles == 32 and rt.lib.rtxh_scene_num_meshes(s._h) == 1


def test_scene_set_mesh_vertices_rejects_and_leaves_the_scene_alone(rt):
    """a wrong vertex count, a changed Vertex.normal.w, an unknown mesh and a null pointer are RTX_ERR_INVALID with a message; the scene is what it was"""
    s = rt.Scene.from_obj([os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "garage.obj"), os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monke.obj")],
                          os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden") + "/")
    assert len(s.meshes) == 2 and s.meshes[1][0][0, 6] != 0           # (the second model's normal.w is its base in materialIDs: not zero)
    before = [read_mesh(rt, s, k).copy() for k in range(2)]
    v = sine_deform(s.meshes[1][0], s.meshes[1][1], 0.05, 9.0, 0.0)
    bad_w = v.copy(); bad_w[3, 6] += 3.0
    for mesh, arr, what in ((1, v[:-1], "count"), (1, np.concatenate([v, v[:1]]), "count"), (1, bad_w, "normal.w"), (2, v, "unknown mesh"), (0, v, "count")):
        with pytest.raises(rt.RtxError) as ei:
            s.set_mesh_vertices(mesh, arr)
        assert what in str(ei.value), (what, str(ei.value))
    assert rt.lib.rtxh_scene_set_mesh_vertices(s._h, 1, None, len(v)) == -1 and b"null" in rt.lib.rtxh_last_error()
    for k in range(2):
        assert np.array_equal(bits(read_mesh(rt, s, k)), bits(before[k])) and np.array_equal(bits(s.meshes[k][0]), bits(before[k]))
    s.set_mesh_vertices(1, v)                                         # and the valid update still goes through
    assert np.array_equal(bits(read_mesh(rt, s, 1)), bits(v))


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
CONFIGS = {"default": ("atrium", []), "host_refit": ("atrium", [("OPT_GPU_REFIT", 0)]), "gpu_build": ("atrium", [("OPT_GPU_BUILD", 1)]), "cornell": ("cornell", [])}


@pytest.mark.gpu
@pytest.mark.parametrize("config", list(CONFIGS))
def test_parity_after_every_vertex_update(rt, world, config):
    """Four successive deformations (monke by a sine along its normals, normals re-derived; one step also bends an emissive mesh, one the atrium itself): after every commit
    the resident tree validates, closest / any hits of camera + 20 000 random rays, the light records and a 4-spp GGX + NEE image with its ray counts equal a fresh oracle
    loaded with the deformed arrays, the image equals a fresh context's, and the commit was a refit.  default: host-built tree, k_reflatten + partial GPU refit;
    host_refit: RTX_OPT_GPU_REFIT 0 (host refit + upload); gpu_build: device-built tree; cornell: the 32-triangle tiny-scene path."""
    name, opts = CONFIGS[config]
    c = rt.Context(0)
    for o, v in opts:
        c.set_option(getattr(rt, o), v)
    c.upload(world.scene(name, 0), W / H)
    check_state(rt, c, world.expect(name, 0), (config, "as built"))
    for k, up in enumerate(world.steps[name]):
        for mesh, v in up:
            c.update_mesh_vertices(mesh, v)
        c.commit()
        assert c.stats().bvh_refits == k + 1, (config, k)
        check_state(rt, c, world.expect(name, k + 1), (config, k))
    c.close()


@pytest.mark.gpu
def test_update_errors_leave_the_committed_scene_alone(rt, world):
    """every RTX_ERR_INVALID case (unknown mesh, vertex count, changed normal.w, null pointer) leaves the scene committed and the next render equal to the previous one; a valid
    update needs a commit: a render in between is RTX_ERR_STATE"""
    sc = world.scene("atrium", 0)
    c = rt.Context(0); c.upload(sc, W / H)
    p = rt.Params(**PT)
    c.clear(W, H); c.render(p); first = c.read_accum()
    v = world.steps["atrium"][0][0][1]
    bad_w = v.copy(); bad_w[5, 6] += 1.0
    for mesh, arr in ((len(sc.meshes), v), (MONKE, v[:-1]), (MONKE, bad_w), (LAMP, v)):
        with pytest.raises(rt.RtxError) as ei:
            c.update_mesh_vertices(mesh, arr)
        assert "(-1)" in str(ei.value) and "update_mesh_vertices" in str(ei.value)
    assert rt.lib.rtx_update_mesh_vertices(c._h, MONKE, None, len(v)) == -1
    c.clear(W, H); c.render(p)
    assert np.array_equal(bits(c.read_accum()), bits(first))
    assert np.array_equal(bits(first), bits(world.expect("atrium", 0)["accum"]))
    c.update_mesh_vertices(MONKE, v)
    with pytest.raises(rt.RtxError) as ei:
        c.render(p)
    assert "(-4)" in str(ei.value)
    c.commit(); c.clear(W, H); c.render(p)
    assert np.array_equal(bits(c.read_accum()), bits(world.expect("atrium", 1)["accum"]))
    c.close()


@pytest.mark.gpu
def test_rebuild_policy_follows_the_tree_cost(rt, world):
    """RTX_OPT_DEFORM_REBUILD.  monke scrambled (every vertex displaced by a random vector of the object's extent): under refit (0) the tree's visit cost exceeds its value after
    the build, and is reproducible to the bit — asked twice, and in a second context that did the same; 1 rebuilds (no refit counted, cost == baseline); a threshold just
    above 100 % rebuilds in the same commit, a huge one refits.  The image never changes and equals the oracle's."""
    sc0 = world.scene("atrium", 0)
    mv, mi, _ = sc0.meshes[MONKE]
    v = scramble(mv, mi, 7)
    e = world.expect_scene(sc0.with_meshes([(MONKE, v)]), 77)
    costs, imgs = {}, {}
    for tag, policy in (("refit", 0), ("refit_again", 0), ("rebuild", 1), ("threshold", 101)):
        c = rt.Context(0); c.set_option(rt.OPT_DEFORM_REBUILD, policy); c.upload(sc0, W / H)
        c.update_mesh_vertices(MONKE, v); c.commit()
        refits = c.stats().bvh_refits
        costs[tag] = c.tree_cost()
        assert costs[tag] == c.tree_cost()
        print(tag, "refits", refits, "tree cost now / after build", costs[tag])
        imgs[tag] = check_state(rt, c, e, tag)
        if policy == 0:
            assert refits == 1 and costs[tag][0] > costs[tag][1] > 0.0, (tag, costs[tag])
        else:
            assert refits == 0 and costs[tag][0] == costs[tag][1] > 0.0, (tag, costs[tag])
        if tag == "refit":                                    # the same context: a threshold far away refits again, then one just above 100 % rebuilds
            c.set_option(rt.OPT_DEFORM_REBUILD, 1000000); c.update_mesh_vertices(MONKE, v); c.commit()
            assert c.stats().bvh_refits == 2 and c.tree_cost() == costs[tag]
            c.set_option(rt.OPT_DEFORM_REBUILD, 101); c.update_mesh_vertices(MONKE, v); c.commit()
            assert c.stats().bvh_refits == 0
            again = c.tree_cost()
            assert again[0] == again[1] and again[0] < costs[tag][0]
            check_state(rt, c, e, "refit, then threshold")
        c.close()
    assert np.array_equal(np.float64(costs["refit"]).view(np.uint64), np.float64(costs["refit_again"]).view(np.uint64))
    for tag in imgs:
        assert np.array_equal(bits(imgs[tag]), bits(imgs["refit"])), tag


@pytest.mark.gpu
def test_restir_frame_after_a_vertex_update(rt, orc, world):
    """update, commit, rtx_restir_reset, one ReSTIR frame: the image and the three history buffers equal a fresh oracle's first frame of the deformed scene (a vertex update
    leaves the history alone — no per-vertex motion vectors —, so a caller who wants no ghosting resets it)"""
    c = rt.Context(0); c.upload(world.scene("atrium", 0), W / H)
    p = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=4, flags=0, frame_seed=5)
    c.restir_reset(); c.clear(W, H); c.render_restir(p)                       # a frame of the undeformed scene: history to be forgotten
    for mesh, v in world.steps["atrium"][0]:
        c.update_mesh_vertices(mesh, v)
    c.commit()
    sc1 = world.scene("atrium", 1)
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
def test_deforming_mesh_from_the_cpp_host(rt, orc, golden_dir):
    """Renderer::SetMeshVertices + OnUpdate + OnRender through the facade's C entry points: two path-traced frames on garage.obj + monke.obj with the monkey deforming,
    accumulated, equal the oracle's — which is loaded afresh with each frame's vertices"""
    sc = rt.Scene.from_obj([os.path.join(golden_dir, "garage.obj"), os.path.join(golden_dir, "monke.obj")], golden_dir + "/")
    Wf, Hf = 96, 56
    r = rt.Renderer(Wf, Hf, "deform", 0)
    r.set_scene(sc); r.on_init()
    r.params.max_bounces = 3
    acc_o = np.zeros((Hf, Wf, 4), np.float32)
    v, idx = sc.meshes[1][0], sc.meshes[1][1]
    for k in range(2):
        v = sine_deform(v, idx, 0.08, 7.0 + k, 0.4 * k)
        sc.set_mesh_vertices(1, v)
        r.set_mesh_vertices(1, v)
        r.on_update(); r.on_render()
        o = orc.Oracle().load(sc, Wf / Hf)
        acc_o, _ = o.render(rt.Params(width=Wf, height=Hf, spp=1, sample_base=1, max_bounces=3, nee_samples=1, rr_start=3, frame_seed=k + 1, flags=0), acc_o)
        o.close()
    assert np.array_equal(bits(r.read_accum()), bits(acc_o))
    with pytest.raises(rt.RtxError):
        r.set_mesh_vertices(1, v[:-1])
    r.close()


@pytest.mark.gpu
def test_scene_cache_after_a_vertex_update_is_never_stale(rt, world, tmp_path):
    """after a GPU-side vertex update the host's per-triangle records are stale: rtx_save_scene_cache refuses (RTX_ERR_STATE) instead of writing them.  After a commit that
    rebuilt on the host (RTX_OPT_DEFORM_REBUILD 1) the mirrors are current again: the file round-trips to the oracle's image."""
    c = rt.Context(0); c.upload(world.scene("atrium", 0), W / H)
    up = world.steps["atrium"][0]
    for mesh, v in up:
        c.update_mesh_vertices(mesh, v)
    c.commit()
    path = tmp_path / "deformed.rtxc"
    with pytest.raises(rt.RtxError) as ei:
        c.save_scene_cache(path)
    assert "(-4)" in str(ei.value) and not path.exists()
    c.set_option(rt.OPT_DEFORM_REBUILD, 1)
    for mesh, v in up:
        c.update_mesh_vertices(mesh, v)
    c.commit()
    assert c.stats().bvh_refits == 0
    c.save_scene_cache(path)
    c.close()
    d = rt.Context(0); d.load_scene_cache(path); d.set_camera(*world.scene("atrium", 1).view_proj(W / H))
    check_state(rt, d, world.expect("atrium", 1), "loaded cache")
    d.close()

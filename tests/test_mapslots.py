"""The seven material-map slots through one tiny scene (the Cornell box): a tiny scene leaves its pre-test records for the general path while ANY slot is active on a
material some triangle uses, and the commit that crosses that line — in either direction — rebuilds.  A slot whose activation the commit forgot to compare would render
through stale records, or stay on the general path; either shows here as a frame that is not the never-mapped one bit for bit."""
import numpy as np
import pytest

from test_deform import bits

W = H = 32
PT = dict(width=W, height=H, spp=2, max_bounces=4, nee_samples=1, frame_seed=7)
NONE = np.uint32(0xFFFFFFFF)
TEX = np.array([[[255, 0, 0, 255], [0, 255, 0, 128]], [[128, 128, 255, 0], [255, 255, 255, 255]]], np.uint8)      # 2 x 2: every channel and the alpha byte vary


def frame(rt, c):
    c.clear(W, H)
    c.render(rt.Params(**PT))
    return c.read_accum()


def fused(rt, c):
    k = c.stats().kernel_launches
    return k[rt.K_BOUNCE] > 0 and k[rt.K_SHADE] == 0


def general(rt, c):
    k = c.stats().kernel_launches
    return k[rt.K_BOUNCE] == 0 and k[rt.K_SHADE] > 0


class World:
    """the never-mapped context's frame (computed once, left unchanged), and the two materials the slots are bound to: the non-emitter and the emitter that the most
    primary rays hit"""
    def __init__(self, rt):
        self.scene = rt.Scene.cornell()
        self.mats = np.asarray(self.scene.materials, np.float32)
        _, idx, mid = self.scene.meshes[0]
        self.tri_mat = np.asarray(mid, np.uint32)[0::3]                  # (a triangle's material is the id of its first index entry)
        self.uvs = np.random.default_rng(5).uniform(-1, 2, (len(idx), 2)).astype(np.float32)
        c = rt.Context(0)
        c.upload(self.scene, W / H)
        self.ref = frame(rt, c)
        assert fused(rt, c)
        mat = self.hit_materials(rt, c)[2]
        emits = self.mats[:, 8:11].max(axis=1) > 0
        count = np.bincount(mat[mat >= 0], minlength=len(self.mats))
        self.plain, self.emitter = int(np.argmax(np.where(emits, 0, count))), int(np.argmax(np.where(emits, count, 0)))
        assert count[self.plain] > 0 and count[self.emitter] > 0 and not emits[self.plain] and emits[self.emitter]
        c.close()

    def hit_materials(self, rt, c):
        """-> (rays, hit records, material per primary ray or -1 for a miss)"""
        rays = c.primary_rays(rt.Params(**PT))
        hits = c.trace_closest(rays)
        prim = hits[:, 3].copy().view(np.uint32)
        return rays, hits, np.where(prim == NONE, -1, self.tri_mat[np.minimum(prim, len(self.tri_mat) - 1)].astype(np.int64))

    def context(self, rt):
        """the scene with UVs and the texture, no slot bound: still the never-mapped frame's path"""
        c = rt.Context(0)
        c.upload(self.scene, W / H)
        c.set_mesh_uvs(0, self.uvs); c.set_texture(0, TEX, False); c.commit()
        return c

    def material_of(self, rt, slot):
        return self.emitter if slot == rt.MAP_KE else self.plain

    def probe(self, rt, c, slot):
        """-> (the slot's texture id per primary ray as its probe reports it, material per primary ray)"""
        rays, hits, mat = self.hit_materials(rt, c)
        if slot == rt.MAP_KD:
            ids = c.albedo(hits)[:, 3].copy().view(np.uint32)
        elif slot == rt.MAP_OPACITY:
            ids = c.opacity(hits)[:, 1].copy().view(np.uint32)
        elif slot == rt.MAP_NORMAL:
            ids = c.shading_normal(rays, hits)[:, 3].copy().view(np.uint32)
        elif slot == rt.MAP_KE:
            ids = c.emission(hits)[1]
        else:
            ids = c.specular(hits)[1][:, {rt.MAP_KS: 0, rt.MAP_PR: 1, rt.MAP_PM: 2}[slot]]
        return ids, mat

    def assert_bound(self, rt, c, slot):
        """the slot's probe reports texture 0 on every hit of the slot's material and no texture anywhere else"""
        ids, mat = self.probe(rt, c, slot)
        on = mat == self.material_of(rt, slot)
        assert on.any() and (ids[on] == 0).all() and (ids[~on] == NONE).all(), slot


@pytest.fixture(scope="module")
def world(rt):
    return World(rt)


SLOTS = ("MAP_KD", "MAP_OPACITY", "MAP_NORMAL", "MAP_KS", "MAP_PR", "MAP_PM", "MAP_KE")


@pytest.mark.gpu
@pytest.mark.parametrize("name", SLOTS)
def test_slot_crosses_to_the_general_path_and_back(rt, world, name):
    slot = getattr(rt, name)
    c = world.context(rt)
    assert np.array_equal(bits(frame(rt, c)), bits(world.ref)) and fused(rt, c)
    c.set_material_map(world.material_of(rt, slot), 0, slot); c.commit()
    assert c.stats().bvh_refits == 0                                     # the commit that crosses the line is a rebuild
    world.assert_bound(rt, c, slot)
    frame(rt, c)
    assert general(rt, c)
    c.set_material_map(world.material_of(rt, slot), None, slot); c.commit()
    assert c.stats().bvh_refits == 0                                     # ... and so is the one that crosses it back
    assert np.array_equal(bits(frame(rt, c)), bits(world.ref)) and fused(rt, c)
    ids, _ = world.probe(rt, c, slot)
    assert (ids == NONE).all()
    c.close()


@pytest.mark.gpu
def test_two_slots_of_different_groups(rt, world):
    a, b = rt.MAP_KD, rt.MAP_NORMAL
    single = world.context(rt)
    single.set_material_map(world.plain, 0, b); single.commit()
    want = frame(rt, single)
    assert general(rt, single) and not np.array_equal(bits(want), bits(world.ref))
    single.close()
    c = world.context(rt)
    c.set_material_map(world.plain, 0, a); c.set_material_map(world.plain, 0, b); c.commit()
    world.assert_bound(rt, c, a); world.assert_bound(rt, c, b)
    both = frame(rt, c)
    assert general(rt, c) and not np.array_equal(bits(both), bits(want))
    c.set_material_map(world.plain, None, a); c.commit()
    world.assert_bound(rt, c, b)
    assert (world.probe(rt, c, a)[0] == NONE).all()
    assert np.array_equal(bits(frame(rt, c)), bits(want)) and general(rt, c)
    c.set_material_map(world.plain, None, b); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(world.ref)) and fused(rt, c)
    c.close()


@pytest.mark.gpu
def test_set_materials_drops_every_slot(rt, world):
    c = world.context(rt)
    for name in SLOTS:
        slot = getattr(rt, name)
        c.set_material_map(world.material_of(rt, slot), 0, slot)
    c.commit()
    for name in SLOTS:
        world.assert_bound(rt, c, getattr(rt, name))
    frame(rt, c)
    assert general(rt, c)
    c.set_materials(world.mats); c.commit()
    assert np.array_equal(bits(frame(rt, c)), bits(world.ref)) and fused(rt, c)
    for name in SLOTS:
        assert (world.probe(rt, c, getattr(rt, name))[0] == NONE).all(), name
    c.close()

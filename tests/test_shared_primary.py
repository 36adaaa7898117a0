"""RTX_OPT_SHARED_PRIMARY: on the fused tiny-scene path without jitter the primary hit and its surface are computed once per pixel and
render call and shared by all samples.  The option changes no result: every comparison here is bit for bit on read_accum() and exact on the
three ray counts — option 1 against option 0 on the same context, and against the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def counts(ctx):
    st = ctx.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def render(rt, ctx, p, shared):
    ctx.set_option(rt.OPT_SHARED_PRIMARY, shared)
    ctx.clear(p.width, p.height)
    ctx.render(p)
    return ctx.read_accum(), counts(ctx)


def assert_same(a, b, what):
    (ia, ca), (ib, cb) = a, b
    assert ca == cb, f"{what}: ray counts {ca} != {cb}"
    assert np.array_equal(bits(ia), bits(ib)), f"{what}: {int((bits(ia) != bits(ib)).any(-1).sum())} pixels differ"


@pytest.fixture(scope="module")
def pair(rt, orc, cornell):
    """the default context for a tiny scene (fused kernels) and the oracle, both with the Cornell box"""
    c = rt.Context(0)
    c.upload(cornell, 2.0)
    yield c, orc.Oracle().load(cornell, 2.0)
    c.close()


def set_view(rt, ctx, o, aspect):
    vp = rt.Scene.cornell().view_proj(aspect)
    ctx.set_camera(*vp)
    if o is not None:
        o.set_camera(*vp)


RAGGED = dict(width=100, height=50, spp=3, sample_base=5, frame_seed=99)      # neither side a multiple of 8: blocks hold invalid slots; the view contains the lamp


@pytest.mark.parametrize("flags", [1, 0])
@pytest.mark.parametrize("nee", [0, 1, 4])
@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_shared_primary_equals_per_sample_primary_and_oracle(rt, pair, bounces, nee, flags):
    ctx, o = pair
    p = rt.Params(max_bounces=bounces, nee_samples=nee, flags=flags, **RAGGED)
    set_view(rt, ctx, o, 2.0)
    off = render(rt, ctx, p, 0)
    on = render(rt, ctx, p, 1)
    ref = o.render(p)
    assert on[0][..., :3].max() > 1.0, "no emissive primary hit in the frame"
    assert_same(on, off, "option 1 vs option 0")
    assert_same(on, (ref[0], tuple(ref[1])), "option 1 vs oracle")


def test_jitter_takes_the_per_sample_path(rt, pair):
    ctx, o = pair
    p = rt.Params(max_bounces=8, nee_samples=1, flags=3, **RAGGED)
    set_view(rt, ctx, o, 2.0)
    off = render(rt, ctx, p, 0)
    on = render(rt, ctx, p, 1)
    ref = o.render(p)
    assert_same(on, off, "jitter: option 1 vs option 0")
    assert_same(on, (ref[0], tuple(ref[1])), "jitter: option 1 vs oracle")


def test_shards_with_shared_primary_reassemble_the_unsharded_image(rt, pair):
    ctx, _ = pair
    base = dict(width=200, height=120, spp=2, max_bounces=5, nee_samples=1, flags=1, tile_size=32)
    set_view(rt, ctx, None, 200 / 120)
    whole, wc = render(rt, ctx, rt.Params(**base), 0)
    ctx.set_option(rt.OPT_SHARED_PRIMARY, 1)
    ctx.clear(200, 120)
    tot = np.zeros(3, np.int64)
    for r in range(3):
        ctx.render(rt.Params(shard_rank=r, shard_count=3, **base))
        tot += np.array(counts(ctx), np.int64)
    assert tuple(int(v) for v in tot) == wc
    assert np.array_equal(bits(ctx.read_accum()), bits(whole))


def test_many_batches_share_one_pre_pass(rt, pair):
    ctx, _ = pair
    p = rt.Params(width=64, height=36, spp=6, max_bounces=5, nee_samples=1, flags=1)
    set_view(rt, ctx, None, 64 / 36)
    one = render(rt, ctx, p, 1)
    ctx.set_option(rt.OPT_PATHS_PER_BATCH, 4096)          # 64 x 36 rounds up to 4096 slots: one sample per batch, six batches
    try:
        many = render(rt, ctx, p, 1)
        many_off = render(rt, ctx, p, 0)
    finally:
        ctx.set_option(rt.OPT_PATHS_PER_BATCH, 128 << 20)
    assert_same(many, one, "six batches vs one batch")
    assert_same(many, many_off, "six batches: option 1 vs option 0")


def test_camera_change_between_calls_leaves_no_stale_record(rt, cornell):
    view, proj = cornell.view_proj(2.0)
    view2 = np.array(view, np.float32).copy()
    view2[12:15] += np.array([0.05, -0.03, 0.02], np.float32)      # the translation of the view matrix (same place in either storage order)
    p = rt.Params(width=100, height=50, spp=3, max_bounces=4, nee_samples=1, flags=1)
    a = rt.Context(0); a.upload(cornell, 2.0)
    a.set_camera(view, proj)
    first = render(rt, a, p, 1)
    a.set_camera(view2, proj)
    second = render(rt, a, p, 1)
    a.close()
    b = rt.Context(0); b.upload(cornell, 2.0)
    b.set_camera(view2, proj)
    fresh = render(rt, b, p, 1)
    fresh_off = render(rt, b, p, 0)
    b.close()
    assert not np.array_equal(bits(first[0]), bits(second[0])), "the second camera shows the same image as the first"
    assert_same(second, fresh, "second call vs a fresh context with the second camera")
    assert_same(second, fresh_off, "second call vs option 0")


class XformedScene:
    """a Scene with its instance transforms replaced (same duck type as rt.Scene for Context.upload / Oracle.load)"""
    def __init__(self, base, mats):
        self.materials, self.meshes, self._base = base.materials, base.meshes, base
        self.instances = [(mesh, np.asarray(m, np.float32).reshape(16)) for (mesh, _), m in zip(base.instances, mats)]

    def view_proj(self, aspect):
        return self._base.view_proj(aspect)


@pytest.mark.parametrize("kind", ["rotated_sheared", "mirrored"])
def test_near_hull_flag_travels_through_the_record(rt, orc, cornell, kind):
    """the room that is not axis-aligned (the transform of test_tiny_scene_paths_on_a_skewed_room): NEE segments of primary hits near a hull plane
    must keep the hull faces in their any-hit test, which the shared record tells bounce 0 with one bit"""
    th, ph = 0.37, -0.21
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]]) @ np.array([[1, 0, 0], [0, np.cos(ph), -np.sin(ph)], [0, np.sin(ph), np.cos(ph)]])
    S = np.array([[1.1, 0.15, 0.0], [0.0, 0.9, 0.1], [0.05, 0.0, 1.2]])
    A = R @ S if kind == "rotated_sheared" else np.diag([-1.0, 1.0, 1.0])
    M = np.eye(4); M[:3, :3] = A; M[:3, 3] = (0.5, 0.5, 0.5) - A @ np.array([0.5, 0.5, 0.5]) + (0.02, -0.01, 0.03)   # about the room's centre
    sc = XformedScene(cornell, [M.T.reshape(16)])                      # column-major storage of a column-vector matrix
    c = rt.Context(0)
    c.upload(sc, 16 / 9)
    o = orc.Oracle().load(sc, 16 / 9)
    p = rt.Params(width=112, height=63, spp=3, max_bounces=8, nee_samples=2, flags=1)
    off = render(rt, c, p, 0)
    on = render(rt, c, p, 1)
    c.close()
    ref = o.render(p)
    assert on[1][2] > 0
    assert_same(on, off, "option 1 vs option 0")
    assert_same(on, (ref[0], tuple(ref[1])), "option 1 vs oracle")

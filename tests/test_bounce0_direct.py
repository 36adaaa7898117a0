"""Bounce 0 of shared-primary frames takes its per-path inputs from the path id: k_raygen_shared writes nothing but the queue word, the bounce-0 kernel derives sample,
slot, pixel and seeds from it (exact division by the batch's slot count, real_slot for the passes of rtx_render_adaptive, the pixel packed into the shared record), and
k_accumulate reads the per-block hit mask of the pre-pass.  None of it may change a bit: every comparison here is bit for bit on read_accum() and exact on the three ray
counts — against the per-sample primary path (RTX_OPT_SHARED_PRIMARY 0, which has none of the above) on the same context, and against the CPU oracle."""
import numpy as np
import pytest

from test_adaptive_ref import BASE, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD
from test_gpu_parity import RandomTinyScene, bits

pytestmark = pytest.mark.gpu


def counts(ctx):
    st = ctx.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def render(rt, ctx, p, shared):
    ctx.set_option(rt.OPT_SHARED_PRIMARY, shared)
    try:
        ctx.clear(p.width, p.height)
        ctx.render(p)
        return ctx.read_accum(), counts(ctx)
    finally:
        ctx.set_option(rt.OPT_SHARED_PRIMARY, 1)


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


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("nee", [0, 1, 4])
@pytest.mark.parametrize("bounces", [1, 2, 8])
def test_cornell_ragged_frame_equals_per_sample_path_and_oracle(rt, pair, bounces, nee, flags):
    ctx, o = pair
    p = rt.Params(max_bounces=bounces, nee_samples=nee, flags=flags, **RAGGED)
    set_view(rt, ctx, o, 2.0)
    on = render(rt, ctx, p, 1)
    off = render(rt, ctx, p, 0)
    ref = o.render(p)
    assert on[0][..., :3].max() > 1.0, "no emissive primary hit in the frame"
    assert_same(on, off, "direct bounce 0 vs per-sample primary path")
    assert_same(on, (ref[0], tuple(ref[1])), "direct bounce 0 vs oracle")


def test_shards_of_a_three_way_tiling_reassemble_the_unsharded_image(rt, pair):
    ctx, _ = pair
    base = dict(width=200, height=120, spp=2, max_bounces=5, nee_samples=1, flags=1, tile_size=16)
    set_view(rt, ctx, None, 200 / 120)
    whole, wc = render(rt, ctx, rt.Params(**base), 0)
    ctx.clear(200, 120)
    tot = np.zeros(3, np.int64)
    for r in range(3):
        ctx.render(rt.Params(shard_rank=r, shard_count=3, **base))
        tot += np.array(counts(ctx), np.int64)
    assert tuple(int(v) for v in tot) == wc
    assert np.array_equal(bits(ctx.read_accum()), bits(whole))


def test_sample_index_restarts_in_every_batch(rt, pair):
    ctx, _ = pair
    p = rt.Params(width=64, height=36, spp=7, sample_base=3, max_bounces=5, nee_samples=1, flags=1)
    set_view(rt, ctx, None, 64 / 36)
    one = render(rt, ctx, p, 1)
    ctx.set_option(rt.OPT_PATHS_PER_BATCH, 8192)          # 64 x 36 rounds up to 4096 slots: two samples per batch, four batches (the last one with a single sample)
    try:
        many = render(rt, ctx, p, 1)
        many_off = render(rt, ctx, p, 0)
    finally:
        ctx.set_option(rt.OPT_PATHS_PER_BATCH, 128 << 20)
    assert_same(many, one, "four batches vs one batch")
    assert_same(many, many_off, "four batches: direct bounce 0 vs per-sample primary path")


def test_long_tapered_sub_queues(rt, pair):
    """one workgroup per CU and 4.4 M paths: the sub-queues are tapered and the longest holds more than 64 chunks, so k_raygen_shared takes its rows in more than one tile"""
    ctx, _ = pair
    p = rt.Params(width=256, height=256, spp=68, max_bounces=2, nee_samples=1, flags=1)      # 256 chunks per sample x 68 samples over <= 304 sub-queues
    set_view(rt, ctx, None, 1.0)
    ctx.set_option(rt.OPT_BLOCKS_PER_CU, 1)
    try:
        on = render(rt, ctx, p, 1)
        off = render(rt, ctx, p, 0)
    finally:
        ctx.set_option(rt.OPT_BLOCKS_PER_CU, 0)
    assert on[1][0] == 256 * 256 * 68
    assert_same(on, off, "long sub-queues: direct bounce 0 vs per-sample primary path")


def test_adaptive_pass_over_a_partly_converged_list(rt, pair):
    """after the first pass some chunks have converged: the later passes render a virtual frame whose slots go through real_slot, in the bounce-0 kernel too"""
    ctx, _ = pair
    p = rt.Params(**dict(BASE, flags=1, tile_size=16, spp=1))          # the frame and threshold of test_adaptive.py: converged chunks after the first pass, others at max_spp
    set_view(rt, ctx, None, 2.0)
    out = []
    for shared in (1, 0):
        ctx.set_option(rt.OPT_SHARED_PRIMARY, shared)
        try:
            ctx.clear(p.width, p.height)
            res = ctx.render_adaptive(p, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD)
            out.append((ctx.read_accum(), counts(ctx), (res.passes, res.chunks, res.chunks_converged, res.chunks_at_max, res.pixel_samples)))
        finally:
            ctx.set_option(rt.OPT_SHARED_PRIMARY, 1)
    on, off = out
    assert on[2][0] >= 2 and 0 < on[2][2] < on[2][1], f"the list never was partly converged: {on[2]}"
    assert on[2] == off[2]
    assert_same(on[:2], off[:2], "adaptive: direct bounce 0 vs per-sample primary path")


def test_camera_and_light_move_between_calls_on_one_context(rt, orc, cornell):
    view, proj = cornell.view_proj(2.0)
    view2 = np.array(view, np.float32).copy()
    view2[12:15] += np.array([0.05, -0.03, 0.02], np.float32)      # the translation of the view matrix (same place in either storage order)
    p = rt.Params(width=100, height=50, spp=3, max_bounces=4, nee_samples=2, flags=1)
    a = rt.Context(0); a.upload(cornell, 2.0)
    a.set_camera(view, proj)
    first = render(rt, a, p, 1)
    a.set_camera(view2, proj)
    second = render(rt, a, p, 1)
    o = orc.Oracle().load(cornell, 2.0); o.set_camera(view2, proj)
    ref = o.render(p)
    assert not np.array_equal(bits(first[0]), bits(second[0])), "the second camera shows the same image as the first"
    assert_same(second, (ref[0], tuple(ref[1])), "second camera vs oracle")
    # every instance (the lamp among them) shifted and sheared a little: new records, new light positions, the same context
    moved = []
    for k, (mesh, m) in enumerate(cornell.instances):
        M = np.asarray(m, np.float64).reshape(4, 4).T.copy()
        D = np.eye(4); D[:3, :3] += np.array([[0.0, 0.04, 0.0], [0.0, 0.0, 0.02], [0.03, 0.0, 0.0]]); D[:3, 3] = (0.02, -0.015, 0.01)
        M2 = np.ascontiguousarray((D @ M).T, np.float32).reshape(16)
        a.set_instance_transform(k, M2)
        moved.append((mesh, M2))
    a.commit()
    third = render(rt, a, p, 1)
    third_off = render(rt, a, p, 0)
    a.close()

    class Moved:
        materials, meshes, instances = cornell.materials, cornell.meshes, moved
        view_proj = staticmethod(cornell.view_proj)
    o2 = orc.Oracle().load(Moved, 2.0); o2.set_camera(view2, proj)
    ref2 = o2.render(p)
    assert not np.array_equal(bits(third[0]), bits(second[0])), "the moved scene shows the same image"
    assert_same(third, third_off, "moved scene: direct bounce 0 vs per-sample primary path")
    assert_same(third, (ref2[0], tuple(ref2[1])), "moved scene vs oracle")


def test_random_tiny_scenes_equal_oracle_and_per_sample_path(rt, orc):
    """40 random tiny scenes (seeds apart from those of test_gpu_parity.py), non-jittered so that the shared path is taken"""
    W, H = 64, 40
    bad = []
    for seed in range(40):
        sc = RandomTinyScene(rt, 31000 + seed)
        p = rt.Params(width=W, height=H, spp=3, max_bounces=5, nee_samples=[1, 2, 4][seed % 3], flags=seed & 1, frame_seed=seed, rr_start=3 if seed % 5 else 1, sample_base=1 + seed % 4)
        oa, oc = orc.Oracle().load(sc, W / H).render(p)
        c = rt.Context(0); c.upload(sc, W / H)
        assert c.stats().triangles <= 64
        on = render(rt, c, p, 1)
        off = render(rt, c, p, 0)
        c.close()
        if not (np.array_equal(bits(on[0]), bits(oa)) and on[1] == tuple(oc) and np.array_equal(bits(on[0]), bits(off[0])) and on[1] == off[1]):
            bad.append(seed)
    assert not bad, f"scenes that differ from the oracle or from the per-sample primary path: {bad}"

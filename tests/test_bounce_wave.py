"""The wave-private form of the fused tiny-scene kernel (RTX_OPT_BOUNCE_VARIANT 2): every wave of a workgroup takes 64-entry chunks of the sub-queue from an LDS cursor,
keeps its hits and its NEE shadow rays in buffers of its own and meets the other waves at the bounce boundary only.  It schedules the same work differently and may not
change a bit: every comparison here is bit for bit on read_accum() and exact on the three ray counts — against variants 0 (workgroup-wide hit ring) and 1 (no ring) on
the same context, and against the CPU oracle where stated."""
import numpy as np
import pytest

from test_adaptive_ref import BASE, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD
from test_gpu_parity import RandomTinyScene, bits

pytestmark = pytest.mark.gpu


def counts(ctx):
    st = ctx.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


def render(rt, ctx, p, variant):
    ctx.set_option(rt.OPT_BOUNCE_VARIANT, variant)
    ctx.clear(p.width, p.height)
    ctx.render(p)
    return ctx.read_accum(), counts(ctx)


def assert_same(a, b, what):
    (ia, ca), (ib, cb) = a, b
    assert ca == cb, f"{what}: ray counts {ca} != {cb}"
    assert np.array_equal(bits(ia), bits(ib)), f"{what}: {int((bits(ia) != bits(ib)).any(-1).sum())} pixels differ"


@pytest.fixture(scope="module")
def pair(rt, orc, cornell):
    """one context for a tiny scene (fused kernels) and the oracle, both with the Cornell box"""
    c = rt.Context(0)
    c.upload(cornell, 2.0)
    yield c, orc.Oracle().load(cornell, 2.0)
    c.close()


def set_view(rt, ctx, o, aspect):
    vp = rt.Scene.cornell().view_proj(aspect)
    ctx.set_camera(*vp)
    if o is not None:
        o.set_camera(*vp)


RAGGED = dict(width=100, height=50, spp=3, sample_base=5, frame_seed=99)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("nee", [0, 1, 4])
@pytest.mark.parametrize("bounces", [2, 8])
def test_cornell_ragged_frame_equals_other_variants_and_oracle(rt, pair, bounces, nee, flags):
    """bounces = 2: a launch with a single bounce; 8: Russian roulette and sub-queues shorter than 64 (partial chunks, buffers drained below 64);
    nee = 4: the drain after every NEE slot; nee = 0: no shadow ray at all;
    flags 2, 3 (FLAG_JITTER without / with Lambert-only): no shared primary record, so bounce 0 shades the hits of k_raygen_trace_small — the one form that calls surface() in bounce 0"""
    ctx, o = pair
    p = rt.Params(max_bounces=bounces, nee_samples=nee, flags=flags, **RAGGED)
    set_view(rt, ctx, o, 2.0)
    wave = render(rt, ctx, p, 2)
    ring = render(rt, ctx, p, 0)
    plain = render(rt, ctx, p, 1)
    ref = o.render(p)
    assert_same(wave, ring, "variant 2 vs variant 0")
    assert_same(wave, plain, "variant 2 vs variant 1")
    assert_same(wave, (ref[0], tuple(ref[1])), "variant 2 vs oracle")


def test_long_sub_queues(rt, pair):
    """one workgroup per CU: sub-queues of eight 256-entry chunks, 32 wave chunks dealt to four waves, both buffers filled and emptied many times; also in index order and untapered"""
    ctx, o = pair
    p = rt.Params(width=256, height=128, spp=16, max_bounces=8, nee_samples=1, flags=1)
    set_view(rt, ctx, o, 2.0)
    ref = o.render(p)
    ctx.set_option(rt.OPT_BLOCKS_PER_CU, 1)
    try:
        wave = render(rt, ctx, p, 2)
        ring = render(rt, ctx, p, 0)
        ctx.set_option(rt.OPT_LPT_ORDER, 0)
        ctx.set_option(rt.OPT_TAPER, 0)
        flat = render(rt, ctx, p, 2)
    finally:
        ctx.set_option(rt.OPT_BLOCKS_PER_CU, 0)
        ctx.set_option(rt.OPT_LPT_ORDER, 1)
        ctx.set_option(rt.OPT_TAPER, 1)
    assert_same(wave, ring, "long sub-queues: variant 2 vs variant 0")
    assert_same(wave, (ref[0], tuple(ref[1])), "long sub-queues: variant 2 vs oracle")
    assert_same(flat, wave, "long sub-queues: index order, untapered vs default deal")


def test_frame_smaller_than_one_chunk_per_wave(rt, pair):
    """384 paths over the sub-queues: most waves find the cursor exhausted at once and must still reach every bounce barrier"""
    ctx, o = pair
    p = rt.Params(width=24, height=16, spp=1, max_bounces=5, nee_samples=1, flags=1)
    set_view(rt, ctx, o, 1.5)
    wave = render(rt, ctx, p, 2)
    ring = render(rt, ctx, p, 0)
    ref = o.render(p)
    assert_same(wave, ring, "tiny frame: variant 2 vs variant 0")
    assert_same(wave, (ref[0], tuple(ref[1])), "tiny frame: variant 2 vs oracle")


def test_random_tiny_scenes_equal_variant_0_and_oracle(rt, orc):
    """twenty random tiny scenes (smooth shading, hull guard, flush lamps), nee 1 and 2, the general (non-Lambert) instantiation"""
    W, H = 64, 36
    bad = []
    for seed in range(20):
        sc = RandomTinyScene(rt, 47000 + seed)
        p = rt.Params(width=W, height=H, spp=2, max_bounces=6, nee_samples=1 + (seed & 1), flags=0, frame_seed=seed)
        oa, oc = orc.Oracle().load(sc, W / H).render(p)
        c = rt.Context(0); c.upload(sc, W / H)
        assert c.stats().triangles <= 64
        wave = render(rt, c, p, 2)
        ring = render(rt, c, p, 0)
        c.close()
        if not (np.array_equal(bits(wave[0]), bits(oa)) and wave[1] == tuple(oc) and np.array_equal(bits(wave[0]), bits(ring[0])) and wave[1] == ring[1]):
            bad.append(seed)
    assert not bad, f"scenes that differ from the oracle or from variant 0: {bad}"


def test_shards_of_a_three_way_tiling_reassemble_the_unsharded_image(rt, pair):
    ctx, _ = pair
    base = dict(width=200, height=120, spp=2, max_bounces=5, nee_samples=1, flags=1, tile_size=16)
    set_view(rt, ctx, None, 200 / 120)
    whole, wc = render(rt, ctx, rt.Params(**base), 2)
    ctx.clear(200, 120)
    tot = np.zeros(3, np.int64)
    for r in range(3):
        ctx.render(rt.Params(shard_rank=r, shard_count=3, **base))
        tot += np.array(counts(ctx), np.int64)
    assert tuple(int(v) for v in tot) == wc
    assert np.array_equal(bits(ctx.read_accum()), bits(whole))


def test_adaptive_call_gives_the_same_bits_as_variant_0(rt, pair):
    ctx, _ = pair
    p = rt.Params(**dict(BASE, flags=1, tile_size=16, spp=1))
    set_view(rt, ctx, None, 2.0)
    out = []
    for variant in (2, 0):
        ctx.set_option(rt.OPT_BOUNCE_VARIANT, variant)
        ctx.clear(p.width, p.height)
        res = ctx.render_adaptive(p, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD)
        out.append((ctx.read_accum(), counts(ctx), (res.passes, res.chunks, res.chunks_converged, res.chunks_at_max, res.pixel_samples)))
    wave, ring = out
    assert wave[2] == ring[2]
    assert_same(wave[:2], ring[:2], "adaptive: variant 2 vs variant 0")

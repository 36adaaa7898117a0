"""The slab form of the tiny-scene pre-test (RTX_OPT_SMALL_SLABS, csrc/rtx_traverse.hpp: traverse_small) on the GPU.  A pre-test, looser or tighter, may only change which rays
reach the exact test and never a hit, so the criterion is derived, not measured: closest hits, any-hit answers, images and ray counts are equal BIT FOR BIT with the option on
and off, and equal to the brute-force oracle's."""
import numpy as np
import pytest

import small_slab_scenes as S
from test_bounce_wave import assert_same, counts

pytestmark = pytest.mark.gpu

W, H = 64, 36
ASPECT = W / H


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def scenes(rt, tmp_path_factory):
    return S.all_scenes(rt, tmp_path_factory.mktemp("slabs"))


@pytest.fixture(scope="module")
def world(rt, orc, scenes):
    """per scene one context and one oracle, made on first use and shared by the tests of this module"""
    made = {}

    def get(name):
        if name not in made:
            c = rt.Context(0)
            c.upload(scenes[name][0], ASPECT)
            assert c.stats().triangles <= 64
            made[name] = (c, orc.Oracle().load(scenes[name][0], ASPECT))
        return made[name]
    yield get
    for c, _ in made.values():
        c.close()


def ray_mix(rt, scene, shapes, seed):
    """about 20 000 rays: random ones, rays aimed at corners, edges and just outside the quads, grazing ones; and short segments for the any-hit query"""
    rng = np.random.default_rng(seed)
    lo, hi = (-0.2, 1.2) if shapes is None else (-1.2, 1.2)
    if shapes is None:
        import test_small_slabs_ref as R
        shapes = R.cornell_shapes(scene, scene.small_records()[1])
    aimed = S.aimed_rays(shapes, rng)[:6000]
    graz = S.random_rays(1000, rng, lo, hi); graz[:, 5] = rng.uniform(-2e-4, 2e-4, len(graz)); graz[:, 4:7] /= np.linalg.norm(graz[:, 4:7], axis=1, keepdims=True)
    closest = np.concatenate([S.random_rays(19000 - len(aimed), rng, lo, hi), aimed, graz])
    seg = np.concatenate([S.random_rays(14000, rng, lo, hi, tmax=0.6), S.random_rays(3000, rng, lo, hi, tmax=0.05), aimed[:3000]])
    seg[14000 + 3000:, 7] = rng.uniform(0.02, 2.0, len(seg) - 17000).astype(np.float32)
    return closest, seg


@pytest.mark.parametrize("name", ["cornell", "rects", "perturbed"] + ["records%d" % n for n in S.RECORD_COUNTS])
def test_debug_trace_equals_brute_force(rt, scenes, world, name):
    """record counts 1, 2, 3, 31, 32, 33, 63, 64: an odd count (padding record), a mixed pair, both sides of the 32-bit candidate word"""
    ctx, o = world(name)
    closest, seg = ray_mix(rt, scenes[name][0], scenes[name][1], 100 + len(name))
    want_c = o.trace_closest(closest, mode=0)
    want_a = o.trace_any(seg, mode=0)
    try:
        for slabs in (1, 0):
            ctx.set_option(rt.OPT_SMALL_SLABS, slabs)
            g = ctx.trace_closest(closest)
            assert np.array_equal(bits(g)[:, 3], bits(want_c)[:, 3]), f"{name}, slabs {slabs}: hit triangle ids differ"
            hit = bits(want_c)[:, 3] != 0xFFFFFFFF
            assert np.array_equal(bits(g)[hit], bits(want_c)[hit]), f"{name}, slabs {slabs}: t / u / v differ"
            assert np.array_equal(ctx.trace_any(seg), want_a), f"{name}, slabs {slabs}: any-hit answers differ"
        assert hit.sum() > 100
    finally:
        ctx.set_option(rt.OPT_SMALL_SLABS, 1)


@pytest.mark.parametrize("nee", [1, 2])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("bounces", [1, 2, 3, 8])
@pytest.mark.parametrize("name", ["cornell", "perturbed", "records33"])
def test_frames_equal_with_option_on_and_off(rt, world, name, bounces, flags, nee):
    """one context switched between frames; the fused kernels trace with the open far end (no far-end slack, rayless lanes cleared after the loops)"""
    ctx, o = world(name)
    p = rt.Params(width=W, height=H, spp=4, sample_base=3, frame_seed=17 + bounces, max_bounces=bounces, nee_samples=nee, flags=flags)
    out = []
    try:
        for slabs in (1, 0):
            ctx.set_option(rt.OPT_SMALL_SLABS, slabs)
            ctx.clear(W, H); ctx.render(p)
            out.append((ctx.read_accum(), counts(ctx)))
    finally:
        ctx.set_option(rt.OPT_SMALL_SLABS, 1)
    assert_same(out[0], out[1], f"{name}: slabs on vs off")
    ref = o.render(p)
    assert out[0][1] == tuple(ref[1]), f"{name}: ray counts {out[0][1]} differ from the oracle's {tuple(ref[1])}"
    assert np.array_equal(bits(out[0][0]), bits(ref[0])), f"{name}: the image differs from the oracle's"

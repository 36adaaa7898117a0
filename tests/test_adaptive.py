"""rtx_render_adaptive on the GPU against the float32 emulation of tests/test_adaptive_ref.py (per-sample oracle frames + the criterion of include/rtx.h): read_accum()
bit for bit in x, y, z and w, pixel-samples and chunk counts exact.  Cornell box at 100 x 50 (blocks with invalid slots; at tile_size 32 chunks without a pixel),
tile_size 16 and 32, min 4 / step 4 / max 16, NEE on.  The threshold is chosen and shown non-vacuous on the CPU (test_adaptive_ref.py::test_inputs_are_not_vacuous)."""
import ctypes as C
import numpy as np
import pytest

import test_adaptive_ref as ref
from test_adaptive_ref import BASE, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD, TILES, W, H, ASPECT

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_image(a, b, what):
    d = bits(a) != bits(b)
    assert not d.any(), f"{what}: {int(d.any(-1).sum())} pixels differ (w differs in {int(d[..., 3].sum())})"


def counts(ctx):
    st = ctx.stats()
    return (st.rays_primary, st.rays_extension, st.rays_shadow)


@pytest.fixture(scope="module")
def fused(rt, cornell):
    """the default context of a tiny scene: the fused kernels"""
    c = rt.Context(0)
    c.upload(cornell, ASPECT)
    yield c
    c.close()


@pytest.fixture(scope="module")
def general(rt, cornell):
    """the same box on the general BVH path: k_raygen, the persistent traversal, k_shade"""
    c = rt.Context(0)
    c.set_option(rt.OPT_SMALL_SCENE, 0)
    c.upload(cornell, ASPECT)
    yield c
    c.close()


def adaptive(rt, ctx, flags, ts, max_spp=MAX_SPP, threshold=THRESHOLD, clear=True, **kw):
    p = rt.Params(**dict(BASE, flags=flags, tile_size=ts, spp=77, **kw))        # (spp is ignored)
    if clear:
        ctx.clear(W, H)
    res = ctx.render_adaptive(p, MIN_SPP, STEP_SPP, max_spp, threshold)
    return ctx.read_accum(), res


def check_against_emulation(rt, ctx, flags, ts, what):
    img, res = adaptive(rt, ctx, flags, ts)
    e, want = ref.emulate(flags, ts)
    st = ctx.stats()
    got = dict(passes=res.passes, chunks=res.chunks, chunks_converged=res.chunks_converged, chunks_at_max=res.chunks_at_max, pixel_samples=res.pixel_samples)
    print(what, got)
    assert got == want, what
    assert st.rays_primary == want["pixel_samples"] and st.paths == want["pixel_samples"], what
    same_image(img, e.accum, what)
    assert st.kernel_launches[rt.K_ADAPT] == 2 * (want["passes"] + 1), "criterion + list once per pass and once to find nothing left"


@pytest.mark.parametrize("ts", TILES)
@pytest.mark.parametrize("shared", [1, 0])
def test_fused_path_matches_the_emulation(rt, fused, shared, ts):
    fused.set_option(rt.OPT_SHARED_PRIMARY, shared)
    try:
        check_against_emulation(rt, fused, 1, ts, f"fused, shared primary {shared}, tile {ts}")
    finally:
        fused.set_option(rt.OPT_SHARED_PRIMARY, 1)


@pytest.mark.parametrize("ts", TILES)
@pytest.mark.parametrize("interleave,compact", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_general_path_matches_the_emulation(rt, general, interleave, compact, ts):
    general.set_option(rt.OPT_SAMPLE_INTERLEAVE, interleave)
    general.set_option(rt.OPT_COMPACT_STATE, compact)
    try:
        check_against_emulation(rt, general, 1, ts, f"general, interleave {interleave}, compact {compact}, tile {ts}")
    finally:
        general.set_option(rt.OPT_SAMPLE_INTERLEAVE, 1)
        general.set_option(rt.OPT_COMPACT_STATE, 1)


@pytest.mark.parametrize("path", ["fused", "general"])
def test_threshold_zero_is_rtx_render_at_max_spp(rt, fused, general, path):
    ctx = fused if path == "fused" else general
    for ts in TILES:
        img, res = adaptive(rt, ctx, 1, ts, threshold=0.0)
        got = counts(ctx)
        ctx.clear(W, H)
        ctx.render(rt.Params(**dict(BASE, flags=1, tile_size=ts, spp=MAX_SPP)))
        same_image(img, ctx.read_accum(), f"{path}, tile {ts}")
        assert got == counts(ctx), f"{path}, tile {ts}: ray counts"
        assert res.chunks_converged == 0 and res.chunks_at_max == res.chunks == 28 and res.pixel_samples == W * H * MAX_SPP and res.passes == 4


@pytest.mark.parametrize("path", ["fused", "general"])
def test_a_later_call_continues_where_the_last_one_stopped(rt, fused, general, path):
    ctx = fused if path == "fused" else general
    for ts in TILES:
        whole, rw = adaptive(rt, ctx, 1, ts)
        first, r1 = adaptive(rt, ctx, 1, ts, max_spp=8)
        both, r2 = adaptive(rt, ctx, 1, ts, clear=False)
        assert not np.array_equal(bits(first), bits(whole)) and r1.chunks_at_max > 0
        same_image(both, whole, f"{path}, tile {ts}: max 8 then max 16 vs max 16")
        assert r1.pixel_samples + r2.pixel_samples == rw.pixel_samples and r1.passes + r2.passes == rw.passes
        assert (r2.chunks_converged, r2.chunks_at_max) == (rw.chunks_converged, rw.chunks_at_max)
        e, _ = ref.emulate(1, ts)
        same_image(both, e.accum, f"{path}, tile {ts}: continued vs emulation")


@pytest.mark.parametrize("path", ["fused", "general"])
@pytest.mark.parametrize("block_tiles", [0, 1])
def test_three_shards_reassemble_the_unsharded_image(rt, fused, general, path, block_tiles):
    ctx = fused if path == "fused" else general
    fl = 1 | (rt.FLAG_BLOCK_TILES if block_tiles else 0)
    for ts in TILES:
        whole, rw = adaptive(rt, ctx, 1, ts)
        ctx.clear(W, H)
        tot = np.zeros(3, np.int64)
        for r in range(3):
            _, rs = adaptive(rt, ctx, fl, ts, clear=False, shard_rank=r, shard_count=3)
            tot += (rs.pixel_samples, rs.chunks_converged, rs.chunks_at_max)
        same_image(ctx.read_accum(), whole, f"{path}, tile {ts}, block tiles {block_tiles}")
        assert tuple(tot) == (rw.pixel_samples, rw.chunks_converged, rw.chunks_at_max)


@pytest.mark.parametrize("path", ["fused", "general"])
def test_passes_split_into_several_batches(rt, fused, general, path):
    ctx = fused if path == "fused" else general
    one, r1 = adaptive(rt, ctx, 1, 16)
    ctx.set_option(rt.OPT_PATHS_PER_BATCH, 4096)          # the first pass has 28 x 256 = 7 168 slots: one sample per batch, four batches; the later passes 1 - 4 batches
    try:
        many, rm = adaptive(rt, ctx, 1, 16)
    finally:
        ctx.set_option(rt.OPT_PATHS_PER_BATCH, 128 << 20)
    same_image(many, one, path)
    assert (r1.passes, r1.pixel_samples, r1.chunks_converged) == (rm.passes, rm.pixel_samples, rm.chunks_converged)


@pytest.mark.parametrize("ts", TILES)
def test_jitter_takes_the_per_sample_primary_path(rt, fused, general, ts):
    check_against_emulation(rt, fused, 3, ts, f"fused, jitter, tile {ts}")
    check_against_emulation(rt, general, 3, ts, f"general, jitter, tile {ts}")


def test_errors_leave_the_image_untouched(rt, fused):
    ctx = fused
    p = rt.Params(**dict(BASE, flags=1, tile_size=16))
    before, _ = adaptive(rt, ctx, 1, 16, max_spp=8)

    def rc(mn, stp, mx, thr=THRESHOLD):
        a = rt.Adaptive(mn, stp, mx, thr, 0.0)
        return rt.lib.rtx_render_adaptive(ctx._h, C.byref(p), C.byref(a), None)
    INVALID, STATE = -1, -4
    for mn, stp, mx in ((3, 4, 16), (0, 4, 16), (4, 3, 16), (4, 0, 16), (4, 1, 16), (8, 4, 6)):
        assert rc(mn, stp, mx) == INVALID, (mn, stp, mx)
    assert rc(4, 4, 16, -1.0) == INVALID and rc(4, 4, 16, float("nan")) == INVALID
    same_image(ctx.read_accum(), before, "after the invalid calls")
    assert rc(4, 4, 8) == rt.RTX_OK                        # nothing left to do at max 8, and no error
    same_image(ctx.read_accum(), before, "after a call with nothing to do")
    ctx.render(p.copy(spp=2, sample_base=40))
    mixed = ctx.read_accum()
    assert rc(4, 4, 16) == STATE                           # u1 holds samples its second sum does not
    with pytest.raises(rt.RtxError):
        ctx.render_adaptive(p, 4, 4, 16, THRESHOLD)
    same_image(ctx.read_accum(), mixed, "after the refused call")
    img, _ = adaptive(rt, ctx, 1, 16)                      # rtx_clear_accum makes it whole again
    same_image(img, ref.emulate(1, 16)[0].accum, "after the clear")

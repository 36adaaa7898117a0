"""The fused tiny-scene kernels with their path state by queue position in two sets (RTX_OPT_COMPACT_STATE 1, the default) against the state by path id, updated in place (0).
The layout moves bytes, not arithmetic: bounce b reads set b & 1 at the entry's place in its sub-queue and writes a survivor into the other set at its slot in the next queue;
radiance additions, their order, the counters and the queues' contents are the same.  So the criterion is derived, not measured: the accumulation buffer is equal BIT FOR BIT
and the three ray counts are equal exactly, in every case below.  Where the CPU oracle is compared too, it is the comparison of the existing tiny-scene tests (bits and counts)."""
import numpy as np
import pytest

from test_adaptive_ref import BASE, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD
from test_bounce_wave import assert_same, counts, set_view
from test_gpu_parity import RandomTinyScene, bits

pytestmark = pytest.mark.gpu

W, H = 150, 90                  # 13 500 pixels = 52.7 chunks of 256: the last chunk and the last wave are partial
ASPECT = W / H
FLAG_JITTER = 2                 # (RTX_FLAG_JITTER: no shared primary record, bounce 0 reads the hit buffer and the state k_raygen_trace_small wrote by path id)


def render(rt, ctx, p, compact, variant=2):
    ctx.set_option(rt.OPT_COMPACT_STATE, compact)
    ctx.set_option(rt.OPT_BOUNCE_VARIANT, variant)
    ctx.clear(p.width, p.height)
    ctx.render(p)
    return ctx.read_accum(), counts(ctx)


@pytest.fixture(scope="module")
def pair(rt, orc, cornell):
    """one context for a tiny scene (fused kernels) and the oracle, both with the Cornell box; every test leaves the context at the default options"""
    c = rt.Context(0)
    c.upload(cornell, ASPECT)
    yield c, orc.Oracle().load(cornell, ASPECT)
    c.close()


@pytest.fixture(autouse=True)
def default_options(rt, pair):
    yield
    pair[0].set_option(rt.OPT_COMPACT_STATE, 1)
    pair[0].set_option(rt.OPT_BOUNCE_VARIANT, 2)


@pytest.mark.parametrize("bounces", [1, 2, 3, 8])
@pytest.mark.parametrize("nee", [0, 1, 4])
@pytest.mark.parametrize("jitter", [0, 1])
@pytest.mark.parametrize("lambert", [0, 1])
def test_ragged_cornell_frame(rt, pair, lambert, jitter, nee, bounces):
    """bounces = 1: bounce 0's output is never read (and never written); 2: a launch of bounces >= 1 with one bounce, which reads set 1; 3 and 8: both parities, Russian roulette,
    sub-queues shorter than a wave.  jitter: bounce 0 starts from the hit buffer (state by path id in set 0) instead of the shared records"""
    ctx, o = pair
    p = rt.Params(width=W, height=H, spp=3, sample_base=5, frame_seed=99, max_bounces=bounces, nee_samples=nee, flags=lambert | (FLAG_JITTER if jitter else 0))
    set_view(rt, ctx, o, ASPECT)
    by_pos = render(rt, ctx, p, 1)
    in_place = render(rt, ctx, p, 0)
    ref = o.render(p)
    assert_same(by_pos, in_place, "by queue position vs in place")
    assert_same(by_pos, (ref[0], tuple(ref[1])), "by queue position vs oracle")


def test_frame_smaller_than_one_chunk_per_wave(rt, pair):
    """120 paths: most sub-queues are empty and most waves find the cursor exhausted at once"""
    ctx, o = pair
    p = rt.Params(width=12, height=10, spp=1, max_bounces=8, nee_samples=1, flags=1)
    set_view(rt, ctx, o, 1.2)
    by_pos = render(rt, ctx, p, 1)
    in_place = render(rt, ctx, p, 0)
    ref = o.render(p)
    assert_same(by_pos, in_place, "tiny frame: by queue position vs in place")
    assert_same(by_pos, (ref[0], tuple(ref[1])), "tiny frame: by queue position vs oracle")


def test_tapered_sub_queues(rt, pair):
    """one sub-queue per CU and at least four chunks for each: the deal is tapered, qcap is the LONGEST sub-queue and exceeds the even share, so a sub-queue's entries lie at
    positions that differ from every path id in it from the first entry on (256 x 144 has 144 chunks per sample; 256 CUs: 8 spp, 1 152 chunks)"""
    import torch
    ctx, o = pair
    G = torch.cuda.get_device_properties(0).multi_processor_count
    spp = max(1, -(-4 * G // 144))
    p = rt.Params(width=256, height=144, spp=spp, max_bounces=8, nee_samples=1, flags=1)
    set_view(rt, ctx, o, 256 / 144)
    ctx.set_option(rt.OPT_BLOCKS_PER_CU, 1)
    try:
        by_pos = render(rt, ctx, p, 1)
        in_place = render(rt, ctx, p, 0)
        ctx.set_option(rt.OPT_TAPER, 0)
        flat = render(rt, ctx, p, 1)
    finally:
        ctx.set_option(rt.OPT_BLOCKS_PER_CU, 0)
        ctx.set_option(rt.OPT_TAPER, 1)
    ref = o.render(p)
    assert_same(by_pos, in_place, "tapered: by queue position vs in place")
    assert_same(by_pos, flat, "tapered vs even deal, both by queue position")
    assert_same(by_pos, (ref[0], tuple(ref[1])), "tapered: by queue position vs oracle")


@pytest.mark.parametrize("jitter", [0, 1])
def test_two_and_three_batches(rt, pair, jitter):
    """150 x 90 at tile_size 16 is 60 tiles = 15 360 slots per sample: RTX_OPT_PATHS_PER_BATCH 30 720 splits 5 spp into 2 + 2 + 1 and 4 spp into 2 + 2 — the sets are reused
    by batches of different length"""
    ctx, _ = pair
    set_view(rt, ctx, None, ASPECT)
    for spp in (5, 4):
        p = rt.Params(width=W, height=H, spp=spp, max_bounces=8, nee_samples=1, flags=1 | (FLAG_JITTER if jitter else 0), tile_size=16)
        whole = render(rt, ctx, p, 1)
        ctx.set_option(rt.OPT_PATHS_PER_BATCH, 2 * 15360)
        try:
            by_pos = render(rt, ctx, p, 1)
            in_place = render(rt, ctx, p, 0)
        finally:
            ctx.set_option(rt.OPT_PATHS_PER_BATCH, 128 << 20)
        assert_same(by_pos, in_place, f"{spp} spp in batches of 2: by queue position vs in place")
        assert by_pos[1] == whole[1], f"{spp} spp in batches of 2 vs one batch: ray counts"


@pytest.mark.parametrize("compact", [0, 1])
def test_shards_of_a_three_way_tiling_reassemble_the_unsharded_image(rt, pair, compact):
    ctx, _ = pair
    base = dict(width=W, height=H, spp=2, max_bounces=5, nee_samples=1, flags=1, tile_size=16)
    set_view(rt, ctx, None, ASPECT)
    whole, wc = render(rt, ctx, rt.Params(**base), compact)
    ctx.clear(W, H)
    tot = np.zeros(3, np.int64)
    for r in range(3):
        ctx.render(rt.Params(shard_rank=r, shard_count=3, **base))
        tot += np.array(counts(ctx), np.int64)
    assert tuple(int(v) for v in tot) == wc
    assert np.array_equal(bits(ctx.read_accum()), bits(whole))


def test_adaptive_call_gives_the_same_bits_in_both_layouts(rt, pair):
    """the list passes render virtual frames with their own slot count: the sets are sized and dealt per pass"""
    ctx, _ = pair
    p = rt.Params(**dict(BASE, width=W, height=H, flags=1, tile_size=16, spp=1))
    set_view(rt, ctx, None, ASPECT)
    out = []
    for compact in (1, 0):
        ctx.set_option(rt.OPT_COMPACT_STATE, compact)
        ctx.clear(p.width, p.height)
        res = ctx.render_adaptive(p, MIN_SPP, STEP_SPP, MAX_SPP, THRESHOLD)
        out.append((ctx.read_accum(), counts(ctx), (res.passes, res.chunks, res.chunks_converged, res.chunks_at_max, res.pixel_samples)))
    by_pos, in_place = out
    assert by_pos[2] == in_place[2]
    assert by_pos[2][0] > 1, "the call must have had list passes"
    assert_same(by_pos[:2], in_place[:2], "adaptive: by queue position vs in place")


def test_one_context_switching_layout_variant_and_size_between_frames(rt, cornell):
    """every frame of the sequence equals the same frame from a fresh context: the buffers are re-sized per frame and no stale set is read.  A block-scheduled form of
    bounces >= 1 (variants 0 and 1) runs the whole frame in place whatever the layout option says"""
    small, big = (64, 48), (W, H)
    seq = [(small, 1, 2), (big, 0, 2), (big, 1, 0), (big, 1, 2), (small, 1, 1), (big, 0, 1), (big, 1, 2), (small, 0, 2), (big, 1, 2)]
    def frame(ctx, size, compact, variant, jitter):
        p = rt.Params(width=size[0], height=size[1], spp=2, max_bounces=8, nee_samples=1, flags=1 | (FLAG_JITTER if jitter else 0), frame_seed=7)
        set_view(rt, ctx, None, size[0] / size[1])
        return render(rt, ctx, p, compact, variant)
    for jitter in (0, 1):
        ctx = rt.Context(0); ctx.upload(cornell, ASPECT)
        got = [frame(ctx, *s, jitter) for s in seq]
        ctx.close()
        for k, s in enumerate(seq):
            fresh = rt.Context(0); fresh.upload(cornell, ASPECT)
            want = frame(fresh, *s, jitter)
            fresh.close()
            assert_same(got[k], want, f"frame {k} {s} jitter {jitter}: switching context vs fresh context")
        for k in range(1, len(seq)):
            if seq[k][0] == seq[1][0]:
                assert_same(got[k], got[1], f"frame {k} {seq[k]} vs frame 1 {seq[1]}, jitter {jitter}")


def test_random_tiny_scenes(rt, orc):
    """random tiny scenes (smooth shading, hull guard, flush lamps), the general (non-Lambert) instantiation, nee 1 and 2; the last one through a thin lens (no shared primary
    record: bounce 0 starts from the hit buffer)"""
    Wr, Hr = 64, 48
    seeds = range(47000, 47006)
    bad = []
    for seed in seeds:
        sc = RandomTinyScene(rt, seed)
        p = rt.Params(width=Wr, height=Hr, spp=2, max_bounces=6, nee_samples=1 + (seed & 1), flags=0, frame_seed=seed)
        lens = seed == seeds[-1]
        c = rt.Context(0); c.upload(sc, Wr / Hr)
        assert c.stats().triangles <= 64
        if lens:
            c.set_lens(0.05, 2.0)
        by_pos = render(rt, c, p, 1)
        in_place = render(rt, c, p, 0)
        c.close()
        same = np.array_equal(bits(by_pos[0]), bits(in_place[0])) and by_pos[1] == in_place[1]
        if same and not lens:
            oa, oc = orc.Oracle().load(sc, Wr / Hr).render(p)
            same = np.array_equal(bits(by_pos[0]), bits(oa)) and by_pos[1] == tuple(oc)
        if not same:
            bad.append(seed)
    assert not bad, f"scenes whose layouts differ (or differ from the oracle): {bad}"

"""Lanes without an item in the fused tiny-scene kernels (csrc/rtx_k_bounce_small.hpp, rtx_k_bounce_wave.hpp).  Such a lane holds UNSPECIFIED values (rtx_shade.hpp:
unspecified<T>(): whatever its registers held) and runs beside the lanes that have an item through the pre-test loop, the ballots and the compactions.  What can go wrong is
such a value leaking into a result, a counter or an address.  It shows where idle lanes are the majority — frames of 1, 63, 64 and 65 entries per sub-queue — and on a second use
of the same context, when registers and LDS hold something else.

The criterion is derived, not measured: nothing that reaches memory may depend on an idle lane, so image and ray counts equal the CPU oracle's BIT FOR BIT (as
tests/test_small_slabs.py compares them), and a frame rendered again after an unrelated frame (other size, seed and flags) on the same context comes back bit-equal.

Cases.  The axes are frame size x samples (5 x 2), the three schedule options (bounce variant 0 / 1 / 2, path state by queue position or in place, shared primary on / off:
12 combinations) and the shading configuration (scene x bounces x flags x NEE samples: 40, of which the 8 with nee_samples 0 run on a scene without lights).  The full
product is 4 800 frames; two cuts of it are run:
  * every size x samples x schedule (120 cases), the 40 shading configurations dealt over them three times each in a fixed shuffled order;
  * every schedule x shading configuration (480 frames in 12 cases) at 13 x 5 pixels and 4 samples: sub-queues of 65 entries, a full wave plus one lane."""
import itertools
import random

import numpy as np
import pytest

import small_slab_scenes as S
from test_bounce_wave import assert_same, counts

pytestmark = pytest.mark.gpu

ASPECT = 64 / 36                # one projection for every frame size: the pixel grid only samples it
SIZES = [(1, 1), (7, 9), (8, 8), (13, 5), (64, 36)]
SPPS = [1, 4]
SCHEDULES = list(itertools.product((0, 1, 2), (0, 1), (0, 1)))                     # (RTX_OPT_BOUNCE_VARIANT, RTX_OPT_COMPACT_STATE, RTX_OPT_SHARED_PRIMARY)
SHADINGS = ([(sc, b, fl, nee) for sc in ("cornell", "records33") for b in (1, 2, 3, 8) for fl in (0, 1) for nee in (1, 2)]
            + [("dark33", b, fl, 0) for b in (1, 2, 3, 8) for fl in (0, 1)])         # dark33: the 33 records with no emissive material
FRAMES = list(itertools.product(SIZES, SPPS, SCHEDULES))
DEAL = SHADINGS * 3
random.Random(20).shuffle(DEAL)
assert len(DEAL) == len(FRAMES)
DARK_MTL = "newmtl wall\nKd 0.7 0.6 0.5\nnewmtl lamp\nKd 0.2 0.3 0.4\n"


@pytest.fixture(scope="module")
def world(rt, orc, tmp_path_factory):
    """name -> (context, oracle, cache of the oracle's frames); made on first use, shared by every case"""
    d = tmp_path_factory.mktemp("idle")
    rng = np.random.default_rng(11)
    shapes = S.scene_records(rng, 33)
    made = {}

    def scene(name):
        if name == "cornell":
            return rt.Scene.cornell()
        sub = d / name
        sub.mkdir()
        files, mtl_dir = shapes.write(sub, name)
        if name == "dark33":
            (sub / "slabs.mtl").write_text(DARK_MTL)
        sc = rt.Scene.from_obj(files, mtl_dir)
        sc.set_camera((0.0, 0.0, 0.0), (0.0, 0.0, -1.0))       # from inside the cloud of records: a tenth of the camera rays hit one (from outside, 1 in 150): most lanes idle
        return sc

    def get(name):
        if name not in made:
            sc = scene(name)
            c = rt.Context(0)
            c.upload(sc, ASPECT)
            assert c.stats().triangles <= 64
            assert (len(c.lights()) == 0) == (name == "dark33")
            made[name] = (c, orc.Oracle().load(sc, ASPECT), {})
        return made[name]
    yield get
    for c, _, _ in made.values():
        c.close()


def set_schedule(rt, ctx, variant, compact, shared):
    ctx.set_option(rt.OPT_BOUNCE_VARIANT, variant)
    ctx.set_option(rt.OPT_COMPACT_STATE, compact)
    ctx.set_option(rt.OPT_SHARED_PRIMARY, shared)


def frame(ctx, p):
    ctx.clear(p.width, p.height)
    ctx.render(p)
    return ctx.read_accum(), counts(ctx)


def check(rt, world, size, spp, schedule, shading):
    name, bounces, flags, nee = shading
    ctx, o, cache = world(name)
    kw = dict(width=size[0], height=size[1], spp=spp, sample_base=3, frame_seed=17 + bounces, max_bounces=bounces, nee_samples=nee, flags=flags)
    key = tuple(sorted(kw.items()))
    if key not in cache:
        img, cnt = o.render(rt.Params(**kw))
        cache[key] = (img, tuple(cnt))
    what = f"{name} {size[0]}x{size[1]} spp {spp} bounces {bounces} flags {flags} nee {nee} schedule {schedule}"
    try:
        set_schedule(rt, ctx, *schedule)
        first = frame(ctx, rt.Params(**kw))
        assert_same(first, cache[key], what + ": GPU vs oracle")
        frame(ctx, rt.Params(width=37, height=23, spp=2, sample_base=9, frame_seed=4242, max_bounces=5, nee_samples=1, flags=1 - flags))      # an unrelated frame
        assert_same(frame(ctx, rt.Params(**kw)), first, what + ": rendered again after an unrelated frame")
    finally:
        set_schedule(rt, ctx, 2, 1, 1)


@pytest.mark.parametrize("k", range(len(FRAMES)), ids=lambda k: "%dx%d-spp%d-v%d-c%d-s%d-" % (FRAMES[k][0] + (FRAMES[k][1],) + FRAMES[k][2]) + "%s-b%d-f%d-n%d" % DEAL[k])
def test_every_size_and_schedule(rt, world, k):
    size, spp, schedule = FRAMES[k]
    check(rt, world, size, spp, schedule, DEAL[k])


@pytest.mark.parametrize("schedule", SCHEDULES, ids=lambda s: "v%d-c%d-s%d" % s)
def test_every_shading_configuration_at_65_entries(rt, world, schedule):
    for shading in SHADINGS:
        check(rt, world, (13, 5), 4, schedule, shading)


def test_the_deal_covers_every_value_of_every_axis_with_every_schedule_value():
    """the shuffled deal of the first cut is fixed; what it must cover is checked here, not hoped for"""
    for axis in range(4):
        values = {s[axis] for s in SHADINGS}
        for part in range(3):
            for v in {s[part] for s in SCHEDULES}:
                assert {DEAL[k][axis] for k in range(len(FRAMES)) if FRAMES[k][2][part] == v} == values
        for size in SIZES:
            assert {DEAL[k][axis] for k in range(len(FRAMES)) if FRAMES[k][0] == size} == values

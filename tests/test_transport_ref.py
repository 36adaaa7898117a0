"""The float64 estimator twin (tests/transport_ref.py) proved on the CPU, before any GPU is involved:

 (a) its vectorised samplers / evaluators equal the scalar ggx_ref64 ones, its map helpers equal the float32 twins within float32 rounding of the same formula;
 (b) at max_bounces = 1 it agrees with a noise-free integral of the NEE half (environment: midpoint grid of the octahedral square; emitter: its area), for every config;
 (c) under RTX_FLAG_LAMBERT_ONLY the pair (environment NEE + BSDF miss) is unbiased for the integral of f L cos+ V on the reduced scene; under GGX the gap is REPORTED:
     sample_ggx flips directions below the normal and the continuation weight uses the unclamped NdotL, so the estimator's expectation is not that integral — a property
     of the reference's text, not asserted away;
 (d) POWER: every named wrong variant moves some block by at least three of the GPU test's tolerances (so tests/test_transport.py would fail on such a kernel);
 (e) the tails are tame: the two halves of the fixture's samples give the same standard deviation within its own standard error (fourth moment);
 (f) the committed fixture is fresh: scene hashes match and a handful of blocks recomputed at reduced n are consistent with it.
"""
import math
import os

import numpy as np
import pytest

import cutout_ref as cr
import env_ref as er
import ggx_ref64 as R
import normalmap_ref as nr
import texture_ref as tr
import transport_ref as tf
import transport_scene as ts

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_ref.npz")
U64, U32 = 2.0 ** -53, 2.0 ** -24
MODES = (("ggx", 0), ("lambert", tf.LAMBERT_ONLY))
# the config on which a wrong variant is exercised (where more than one applies: the one with the fewest other features)
APPLIES = {"n_geometric_in_nee": "env+kd+nrm", "n_geometric_in_continuation": "env+kd+nrm", "n_geometric_in_view_terms": "env+kd+nrm",
           "kd_untextured_in_env_nee": "env+kd", "kd_untextured_in_light_nee": "kd+nrm", "kd_untextured_in_continuation": "env+kd",
           "no_mis_env_nee": "env", "no_mis_env_miss": "env", "r3_of_texel_centre": "env", "texture_nearest": "env+kd",
           "green_flipped": "env+kd+nrm", "handedness_ignored": "env+kd+nrm",
           "cutout_ignored_by_shadow_rays": "env+kd+nrm+cut", "cutout_ignored_by_closest_hit": "env+kd+nrm+cut", "env_rotation_transposed": "env"}
POWER_BLOCKS = ((2, 2), (7, 5), (5, 5), (1, 4), (0, 2), (4, 3))      # (column, row): wall, floor and seam blocks; a subset can only lower the maximum


class World:
    def __init__(self, rt, orc):
        self.scene, self.rays, self.blocks = {}, {}, {}
        for cfg in ts.CONFIGS:
            s = ts.build(rt, cfg)
            self.scene[cfg], self.rays[cfg] = s, ts.primary_rays(orc, rt, s)
            self.blocks[cfg] = ts.Blocks(tf.Twin(s), self.rays[cfg])
        self.fixture = np.load(FIXTURE)

    def tol(self, cfg, fi, bx, by):
        """the GPU test's tolerance for block (bx, by): (max_bounces, 3)"""
        ci = ts.CONFIGS.index(cfg)
        return ts.tolerance(self.fixture["std"][ci, fi, :, by, bx].astype(np.float64), self.fixture["mean"][ci, fi, :, by, bx], ts.N_GPU, int(self.fixture["n"]))


@pytest.fixture(scope="module")
def world(rt, orc):
    return World(rt, orc)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------
# (a) the twin's pieces against the existing witnesses
# ------------------------------------------------------------------------------------------------
def test_vectorised_bsdf_equals_the_scalar_restatement(rt):
    """Same formulas, evaluated on arrays: the operations differ at most in association (np.cross, sums over the last axis).  A sampled direction is a unit vector reached
    through about 90 float64 operations on values of magnitude <= 1, each rounding <= 2^-53, through four normalisations whose shortest input here is >= 0.05 (alpha^2 =
    0.04 stretch of a unit vector): 90 x 2^-53 x 20 = 2e-13.  The mixture repeats ggx_ref64.mixture's operations one for one: 16 ulp relative."""
    rng = np.random.default_rng(5)
    k = 400
    n = unit(rng.normal(size=(k, 3)))
    n[:8] = [(0, 0, 1), (0, 0, -1), (0.02, 0.0, 0.9998), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0.6, 0, 0.8), (0, 0.0447101778, 0.999)]
    n = unit(n)
    wo = unit(n + 0.9 * unit(rng.normal(size=(k, 3))))
    u = rng.random((k, 3))
    lut = rt.generate_ess_lut(0.45)
    m = R.Mat((0.55, 0.68, 0.74), (0.05, 0.06, 0.08), 0.45, 0.3, lut)
    got_g, got_l = tf.sample_ggx_v(m.Pr, wo, n, u[:, 0], u[:, 1]), tf.sample_lambert_v(n, u[:, 0], u[:, 1])
    T, B = tf.coordinate_system_v(n)
    worst = 0.0
    for i in range(k):
        sg, _ = R.sample_ggx(m, wo[i], n[i], u[i, 0], u[i, 1])
        sl = R.sample_lambert(n[i], u[i, 0], u[i, 1])
        t, b = R.coordinate_system(n[i])
        worst = max(worst, np.abs(got_g[i] - sg).max(), np.abs(got_l[i] - sl).max(), np.abs(T[i] - t).max(), np.abs(B[i] - b).max())
    print("samplers: largest |vectorised - scalar| =", worst)
    assert worst <= 90 * U64 * 20
    L = unit(n + 0.8 * unit(rng.normal(size=(k, 3))))
    kdpi = m.Kd[:3] / R.PI
    F, P = tf.mixture_v(m, n, L, wo, kdpi, False)
    F0, P0, _, _ = R.mixture(m, n, L, wo)
    assert np.isfinite(F0).all() and (P0 > 0).all()
    assert np.abs(F - F0).max() <= 16 * U64 * np.abs(F0).max() and np.abs(P / P0 - 1.0).max() <= 16 * U64
    pd, ps = R.strategy_probs(m, wo, n)
    pick = np.where(u[:, 2] <= ps, 1, 0)
    assert np.array_equal(pick, R.select_strategy(m, wo, n, u[:, 2])) and 0 < pick.sum() < k        # both strategies are drawn
    Fl, Pl = tf.mixture_v(m, n, L, wo, kdpi, True)
    assert np.array_equal(Fl, np.broadcast_to(R.lambert_eval(m), Fl.shape)) and np.array_equal(Pl, R.lambert_pdf(n, L))


def test_map_helpers_equal_the_float32_twins(rt):
    """float64 restatements against the float32 twins of the same rtx.h text.  Sample(): the texel coordinate x = fs W - 0.5 carries <= (1 + |s|) W 2^-24 of float32 rounding
    and the bilinear value moves by at most one table step (<= 1) per texel of x; the three lerps add 9 roundings of values <= 1: bound (9 + 2 (1 + |s|max) max(W, H)) 2^-24
    per unit of table range.  n': a unit vector through about 40 float32 operations, conditioned by |m| >= c.z >= 0.7: 64 x 2^-24.  Directions of the map: 24 x 2^-24."""
    rng = np.random.default_rng(9)
    k = 4000
    s, t = rng.uniform(-2.5, 3.5, k).astype(np.float32), rng.uniform(-2.5, 3.5, k).astype(np.float32)
    s64, t64 = s.astype(np.float64), t.astype(np.float64)
    for px, srgb in ((ts.kd_texture(), True), (ts.normal_texture(), False), (ts.alpha_texture(), False)):
        bound = (9 + 2 * 4.5 * max(px.shape[:2])) * U32
        img = tr.table(srgb).astype(np.float64)[px[..., :3]]
        assert np.abs(tf.sample_image(img, s64, t64) - tr.sample(px, srgb, s, t)).max() <= bound
        a64 = tf.sample_image(tr.table(False).astype(np.float64)[px[..., 3:4]], s64, t64)[:, 0]
        assert np.abs(a64 - cr.alpha(px, s, t)).max() <= bound
        c64 = tf.sample_image(nr.table().astype(np.float64)[px[..., :3]], s64, t64)
        assert np.abs(c64 - nr.decode(px, s, t)).max() <= 2.0 * bound                   # the table Nt spans [-1, 1]
        near = tf.sample_image(img, s64, t64, nearest=True)
        assert (np.abs(near[:, None, None, :] - img[None]).min(axis=(1, 2)) == 0).all()  # nearest returns texels, and not the bilinear value
        assert img.max() == 0 or np.abs(near - tf.sample_image(img, s64, t64)).max() > 0.01
    # Kd' = half_round(Kd tl): the float64 product rounds like the float32 one except within 2^-24 of a binary16 tie
    kd = np.array([0.72, 0.66, 0.58], np.float32)
    tl = tr.sample(ts.kd_texture(), True, s, t)
    a, b = tf.kd_prime(R.half(kd)[:3], tl.astype(np.float64)), tr.kd_prime(rt.half_round, kd, tl).astype(np.float64)
    assert (a != b).mean() <= 0.002 and np.abs(a - b).max() <= 2.0 ** -11
    # n' on a mirrored instance with mirrored UVs and without, both viewer sides
    c = nr.decode(ts.normal_texture(), s, t)
    assert not ((c[:, 0] == 0) & (c[:, 1] == 0)).any()
    for mirror_uv in (False, True):
        for mirror_inst in (False, True):
            M3 = ts.rotation((1.0, 2.0, 3.0), 40.0) @ np.diag([-1.0 if mirror_inst else 1.0, 1.0, 1.0])
            o2w = ts.mat16(M3)
            p3 = np.array([[(0, 0, 0), (1, 0, 0), (0, 1, 0)]], np.float32)
            uv3 = np.array([[(0, 0), (0.7, 0.2), (0.3 if mirror_uv else -0.3, -0.9 if mirror_uv else 0.9)]], np.float32)
            tan = nr.tangent_records(p3, uv3)
            n32 = unit((np.linalg.inv(M3.astype(np.float32).astype(np.float64)).T @ np.array([0.0, 0.0, 1.0]))).astype(np.float32)
            wo = unit(n32 + 1.3 * unit(rng.normal(size=(k, 3)))).astype(np.float32)
            br = {}
            want = nr.perturb(np.tile(n32, (k, 1)), c, np.tile(tan, (k, 1)), np.tile(o2w, (k, 1)), wo, br)
            M64 = o2w.astype(np.float64).reshape(4, 4).T[:3, :3]
            t6 = tan[0].astype(np.float64)
            got = tf.perturb_v(n32.astype(np.float64), M64 @ t6[:3], M64 @ t6[3:], c.astype(np.float64), wo.astype(np.float64))
            ap = (want * wo).sum(1)
            away = np.abs(ap) > 1e-4                                                      # off the guard's own threshold, where the two roundings may decide differently
            assert br["guard"].any() and not br["degenerate"].any() and away.mean() > 0.99
            assert np.abs(got - want)[away].max() <= 64 * U32
            flipped = tf.perturb_v(n32.astype(np.float64), M64 @ t6[:3], M64 @ t6[3:], c.astype(np.float64), wo.astype(np.float64), handedness_ignored=True)
            assert (np.abs(flipped - got).max() > 0.1) == (mirror_uv != mirror_inst)      # the handedness sign is -1 exactly when UVs XOR instance are mirrored
    # the environment: lookup, decode and the sampler on the float32 twin's own draws
    img, rot = ts.sky()
    tab, env = er.Tables(img, 1.0, rot), tf.Env(img, rot, 1.0)
    d = unit(rng.normal(size=(k, 3))).astype(np.float32)
    L32, pdf32, tex32, _ = tab.eval(d)
    L64, pdf64 = env.eval(d.astype(np.float64))
    same = (L64 == L32).all(1)                                                            # a direction within rounding of a texel border may land next door
    assert same.mean() >= 0.995 and np.abs(pdf64[same] / np.maximum(pdf32[same], 1e-30) - 1.0)[pdf32[same] > 0].max() <= 24 * U32
    s0, s1 = rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, k, dtype=np.uint64).astype(np.uint32)
    d32, p32, l32, _, _, _ = tab.sample(s0, s1)
    xi = []
    for _ in range(4):
        x, s0, s1 = er.tea_next(s0, s1)
        xi.append(x.astype(np.float64))
    d64, p64, l64 = env.sample(*xi)
    assert np.array_equal(l64, l32.astype(np.float64)) and np.abs(d64 - d32).max() <= 24 * U32 and np.abs(p64 / p32 - 1.0).max() <= 24 * U32
    lit = img.sum(-1) > 0
    assert tab.texels[..., :3].max() / tab.texels[..., :3][lit].mean() <= 8.5             # the balance heuristic keeps the samples bounded


def test_scene_is_what_the_issue_asks_for(world):
    for cfg in ts.CONFIGS:
        b, s = world.blocks[cfg], world.scene[cfg]
        assert sum(len(i) // 3 for _, i, _ in s.meshes) <= 16
        assert b.fraction_left_out() <= 0.25 and len(b.ids) >= 30
        assert set(np.unique(b.hq)) == {-1, 0, 3}                                        # sky, floor, wall: neither the emitter nor the card is in view
        assert all(p in b.ids for p in POWER_BLOCKS)
    quads = tf.quads_of(world.scene["env+kd+nrm+cut"])
    floor, wall = quads[0], quads[3]
    assert abs(floor.N @ wall.N) < 1e-6                                                  # a right angle
    det = lambda Q: np.linalg.det(np.array([Q.uv3[0, 1] - Q.uv3[0, 0], Q.uv3[0, 2] - Q.uv3[0, 0]]))
    sign = lambda Q: np.sign(np.cross(Q.E1, Q.E2) @ Q.N)
    assert det(floor) * sign(floor) * det(wall) * sign(wall) < 0                           # one of the two has mirrored UVs
    assert np.linalg.det(np.asarray(world.scene["env+kd+nrm"].instances[1][1]).reshape(4, 4)[:3, :3]) < 0 < np.linalg.det(np.asarray(world.scene["env"].instances[1][1]).reshape(4, 4)[:3, :3])
    a = ts.alpha_texture()[..., 3]
    assert a.max() > 200 and a[0].max() < 64 and (a[2:-2, 2:-2] < 128).any() and (a[2:-2, 2:-2] >= 128).any()      # the blob crosses 0.5 inside the card


# ------------------------------------------------------------------------------------------------
# (b) max_bounces = 1 against the noise-free NEE-only integral
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", ts.CONFIGS)
def test_one_bounce_equals_the_nee_only_integral(world, config):
    n = 1024
    for fi, (name, flags) in enumerate(MODES):
        tw = tf.Twin(world.scene[config], flags)
        for bx, by in ((2, 2), (5, 5)):                                                  # a wall block and a floor block
            pix = tf.block_pixels(ts.W, bx, by)
            rays = world.rays[config]
            x = tf.block_samples(tw, rays, pix, n, 1, np.random.default_rng([11, fi, bx, by]))[0]
            mean, se = x.mean(0), x.std(0, ddof=1) / math.sqrt(n)
            o, d = rays[pix, 0:3].astype(np.float64), rays[pix, 4:7].astype(np.float64)
            coarse, fine = tf.nee_only_expectation(tw, o, d, 64, 16).mean(0), tf.nee_only_expectation(tw, o, d, 128, 32).mean(0)
            print(f"{config} {name} block {(bx, by)}: twin {mean} +- {se}, integral {fine} (grid halved: {coarse})")
            assert (np.abs(coarse - fine) <= 0.1 * 6.0 * se).all()                       # the grid is converged far below the statistical margin
            assert (np.abs(mean - fine) <= 6.0 * se + np.abs(coarse - fine)).all()
            # ... and so does the committed fixture, whose standard error is eight times smaller
            ci = ts.CONFIGS.index(config)
            fmean, fse = world.fixture["mean"][ci, fi, 0, by, bx], world.fixture["std"][ci, fi, 0, by, bx].astype(np.float64) / math.sqrt(ts.N_REF)
            print(f"    fixture {fmean} +- {fse}: {(fmean - fine) / fse} standard errors from the integral")
            assert (np.abs(fmean - fine) <= 6.0 * fse + np.abs(coarse - fine)).all()


# ------------------------------------------------------------------------------------------------
# (c) the estimator pair against the textbook integral: unbiased under Lambert, a reported gap under GGX
# ------------------------------------------------------------------------------------------------
def test_lambert_pair_is_unbiased_and_the_ggx_gap_is_reported(rt, orc):
    scene = ts.build(rt, "env+kd+nrm+cut", floor_only=True)
    rays = ts.primary_rays(orc, rt, scene)
    n = 1024
    for fi, (name, flags) in enumerate(MODES):
        tw = tf.Twin(scene, flags)
        assert tw.nee == 0 and len(tw.quads) == 2
        for bx, by in ((2, 5), (5, 5)):
            pix = tf.block_pixels(ts.W, bx, by)
            x = tf.block_samples(tw, rays, pix, n, 2, np.random.default_rng([13, fi, bx]))[1]
            mean, se = x.mean(0), x.std(0, ddof=1) / math.sqrt(n)
            o, d = rays[pix, 0:3].astype(np.float64), rays[pix, 4:7].astype(np.float64)
            coarse, fine = tf.direct_integral(tw, o, d, 128).mean(0), tf.direct_integral(tw, o, d, 256).mean(0)
            gap = (mean - fine) / fine
            print(f"{name} block {(bx, by)}: pair {mean} +- {se}, integral of f L cos+ V {fine} (grid halved: {coarse}), relative gap {gap}, in standard errors {(mean - fine) / se}")
            assert (np.abs(coarse - fine) <= 0.25 * 6.0 * se).all()                     # (no MIS weight smooths this integrand: the card's edge converges like 1 / grid)
            if flags:
                assert (np.abs(mean - fine) <= 6.0 * se + np.abs(coarse - fine)).all()


# ------------------------------------------------------------------------------------------------
# (d) power
# ------------------------------------------------------------------------------------------------
_BASE = {}


def _power_samples(world, cfg, wrong, n):
    tw = tf.Twin(world.scene[cfg], 0, wrong)
    return np.stack([tf.block_samples(tw, world.rays[cfg], tf.block_pixels(ts.W, bx, by), n, 3, np.random.default_rng([17, bx, by])) for bx, by in POWER_BLOCKS])


@pytest.mark.parametrize("wrong", tf.WRONG)
def test_every_wrong_variant_would_fail_the_gpu_test(world, wrong):
    """common random numbers between right and wrong (the same generator, the same number of draws per path and bounce), so the DIFFERENCE of the two expectations is
    tight; it is held against the tolerance the GPU test uses, from the fixture's sigma and the GPU test's sample counts.  Asserted on the difference less three of its
    own standard errors."""
    cfg = APPLIES[wrong]
    n = 1024 if wrong in ("r3_of_texel_centre", "cutout_ignored_by_closest_hit") else 192      # the two weakest: more samples for a tight difference
    key = (cfg, n)
    if key not in _BASE:
        _BASE[key] = _power_samples(world, cfg, None, n)
    diff = _power_samples(world, cfg, wrong, n) - _BASE[key]                            # (blocks, max_bounces, n, 3)
    tol = np.stack([world.tol(cfg, 0, bx, by) for bx, by in POWER_BLOCKS])
    shift, se = np.abs(diff.mean(2)), diff.std(2, ddof=1) / math.sqrt(n)
    score, low = (shift / tol).max(), ((shift - 3.0 * se) / tol).max()
    print(f"power {wrong} on {cfg}: largest shift {score:.1f} tolerances (at least {low:.1f})")
    assert low >= 3.0


def test_every_variant_is_named_and_applies_somewhere():
    assert set(APPLIES) == set(tf.WRONG) and set(APPLIES.values()) <= set(ts.CONFIGS)


# ------------------------------------------------------------------------------------------------
# (e) tails, (f) freshness
# ------------------------------------------------------------------------------------------------
def test_fixture_tails_are_tame(world):
    """std of the two halves of the reference samples, per config, mode, bounce count, block and channel: their difference against the standard error of a standard
    deviation at n / 2, SE(s) = sqrt((m4 - s^4) / n) / (2 s), from the sample fourth moment.  A config that fails has inputs too spiky for its n."""
    f = world.fixture
    n = int(f["n"])
    used = f["used"].astype(bool)
    worst = 0.0
    for ci, cfg in enumerate(ts.CONFIGS):
        u = used[ci]
        s, sa, sb, m4 = (f[k][ci][:, :, u].astype(np.float64) for k in ("std", "std_a", "std_b", "m4"))
        assert np.isfinite(s).all() and (s > 0).all()
        se_half = np.sqrt(np.maximum(m4 - s ** 4, 0.0) / (n / 2)) / (2.0 * s)
        z = np.abs(sa - sb) / (math.sqrt(2.0) * se_half)
        kurt = m4 / s ** 4
        print(f"{cfg}: largest |std_a - std_b| = {z.max():.2f} standard errors, largest kurtosis {kurt.max():.1f}")
        worst = max(worst, float(z.max()))
        assert (z <= 6.0).all()
    assert worst > 0.0


def test_fixture_is_fresh(world):
    f = world.fixture
    assert [str(c) for c in f["configs"]] == list(ts.CONFIGS) and int(f["n"]) == ts.N_REF
    for ci, cfg in enumerate(ts.CONFIGS):
        assert str(f["scene_hash"][ci]) == tf.scene_hash(world.scene[cfg]), cfg
        assert np.array_equal(f["used"][ci].astype(bool), world.blocks[cfg].used)
        assert np.isnan(f["mean"][ci][:, :, ~world.blocks[cfg].used]).all()
    n = 512
    for cfg, fi, (bx, by) in (("env+kd+nrm+cut", 0, (3, 2)), ("env+kd+nrm+cut", 1, (6, 5)), ("kd+nrm", 0, (4, 4)), ("env", 1, (1, 1))):
        ci = ts.CONFIGS.index(cfg)
        tw = tf.Twin(world.scene[cfg], MODES[fi][1])
        x = tf.block_samples(tw, world.rays[cfg], tf.block_pixels(ts.W, bx, by), n, 3, np.random.default_rng([19, ci, fi]))
        mean, sd = x.mean(1), x.std(1, ddof=1)
        ref, sig = f["mean"][ci, fi, :, by, bx], f["std"][ci, fi, :, by, bx].astype(np.float64)
        assert (np.abs(mean - ref) <= 6.0 * sig * math.sqrt(1.0 / n + 1.0 / ts.N_REF)).all(), (cfg, fi, bx, by)
        assert (np.abs(sd / sig - 1.0) <= 0.5).all()

"""The transport of the extensions on the device — diffuse maps, normal maps, alpha cut-outs, environment lighting, in k_shade<false / true, TEX, ENV, NRM> and the CUT forms of
the traversal kernels — held to the float64 twin of the estimator (tests/transport_ref.py) through its committed expectations (tests/golden/transport_ref.npz, written by
tests/golden/make_transport_ref.py).  Per 4 x 4 pixel block and channel, for every config x {GGX, Lambert-only} x max_bounces {1, 2, 3}:

    |mean_gpu - mean_ref| <= 6 sigma_ref sqrt(1 / n_gpu + 1 / n_ref) + spp 2^-24 |mean_ref|

sigma_ref is the FIXTURE's per-sample standard deviation, never the GPU's own scatter; the second term bounds the sequential float32 accumulation of spp terms and is the
only systematic allowance.  tests/test_transport_ref.py (no GPU) proves the twin and shows that every named wrong kernel of transport_ref.WRONG would move some block by at
least three of these tolerances.  Out of scope: RTX_FLAG_TRANSMISSION, the thin lens, Russian roulette (rr_start = max_bounces)."""
import os
import time

import numpy as np
import pytest

import env_ref as er
import transport_ref as tf
import transport_scene as ts
from test_deform import bits

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_ref.npz")
MODES = (("ggx", 0), ("lambert", tf.LAMBERT_ONLY))


@pytest.fixture(scope="module")
def fixture():
    return np.load(FIXTURE)


def params(rt, flags, mb, frame, spp=ts.GPU_SPP):
    """frame f: its own range of sample ids and its own frame seed, so that no two frames share a path"""
    return rt.Params(width=ts.W, height=ts.H, spp=spp, sample_base=1 + frame * spp, max_bounces=mb, nee_samples=1, rr_start=mb, frame_seed=1 + frame, flags=flags)


def render_sum(rt, c, flags, mb, frames=ts.GPU_FRAMES, spp=ts.GPU_SPP, first=None):
    """frames x (clear, render spp, read): the float32 accumulator never holds more than spp terms; the frames are summed in float64 on the host.  -> (H, W, 4) sums;
    first (a list, optional) receives the first frame as read and the statistics of its render"""
    tot = np.zeros((ts.H, ts.W, 4), np.float64)
    for f in range(frames):
        c.clear(ts.W, ts.H)
        c.render(params(rt, flags, mb, f, spp))
        img = c.read_accum()
        if f == 0 and first is not None:
            first += [img.copy(), c.stats()]
        tot += img
    return tot


def check_config(rt, orc, fixture, config, opts=()):
    ci = ts.CONFIGS.index(config)
    scene = ts.build(rt, config)
    assert tf.scene_hash(scene) == str(fixture["scene_hash"][ci]), "the fixture was generated for another scene: rerun tests/golden/make_transport_ref.py"
    rays = ts.primary_rays(orc, rt, scene)
    blocks = ts.Blocks(tf.Twin(scene), rays)
    assert blocks.fraction_left_out() <= 0.25 and len(blocks.ids) >= 30
    used = fixture["used"][ci].astype(bool)
    assert np.array_equal(used, blocks.used)
    n_ref = int(fixture["n"])
    env = scene.environment
    c = rt.Context(0)
    images = {}
    try:
        for o, v in opts:
            c.set_option(getattr(rt, o), v)
        c.upload(scene, ts.ASPECT)
        for name, flags in MODES:
            fi = 1 if flags else 0
            for mb in ts.MAX_BOUNCES:
                first = []
                t0 = time.time()
                tot = render_sum(rt, c, flags, mb, first=first)
                img0, st = first
                # the intended form ran: general path (a map or an environment is bound to a tiny scene), one shadow launch per NEE slot and bounce
                assert st.kernel_launches[rt.K_BOUNCE] == 0 and st.kernel_launches[rt.K_SHADE] == mb
                assert st.kernel_launches[rt.K_SHADOW] == (2 if env is not None else 1) * mb
                assert (img0[..., 3] == ts.GPU_SPP).all() and (tot[..., 3] == ts.N_GPU).all()
                # primary misses: exactly spp L(d) with an environment, exactly zero bits without one
                miss = blocks.miss.ravel()
                assert miss.sum() >= ts.W * ts.EDGE
                got = img0.reshape(-1, 4)[miss, :3]
                if env is not None:
                    L = er.Tables(env["img"], env["scale"], env["to_world"]).eval(rays[miss, 4:7])[0]
                    want = np.zeros_like(L)
                    for _ in range(ts.GPU_SPP):
                        want = want + L
                    assert np.array_equal(bits(got), bits(want))
                else:
                    assert not bits(got).any()
                mean_gpu = ts.block_means(tot[..., :3] / float(ts.N_GPU))
                mean_ref, sigma_ref = fixture["mean"][ci, fi, mb - 1], fixture["std"][ci, fi, mb - 1]
                tol = ts.tolerance(sigma_ref[used], mean_ref[used], ts.N_GPU, n_ref)
                ratio = np.abs(mean_gpu[used] - mean_ref[used]) / tol
                print(f"{config} {name} max_bounces={mb}: n_gpu={ts.N_GPU} n_ref={n_ref} largest |diff| / tol = {ratio.max():.3f} over {used.sum()} blocks x 3 channels, "
                      f"{time.time() - t0:.2f} s")
                assert (ratio <= 1.0).all(), (config, name, mb, float(ratio.max()), np.argwhere(ratio > 1.0)[:8].tolist())
                images[(name, mb)] = img0
    finally:
        c.close()
    return images


@pytest.mark.parametrize("config", ts.CONFIGS)
def test_converged_frames_match_the_estimator_twin(rt, orc, fixture, config):
    check_config(rt, orc, fixture, config)


def test_full_stack_is_the_same_bits_in_both_state_layouts(rt, orc):
    """RTX_OPT_COMPACT_STATE 0 against the default on the full-stack config, one frame each: ties the energy result to both layouts of the path state"""
    scene = ts.build(rt, "env+kd+nrm+cut")
    out = []
    for opts in ((), (("OPT_COMPACT_STATE", 0),)):
        c = rt.Context(0)
        try:
            for o, v in opts:
                c.set_option(getattr(rt, o), v)
            c.upload(scene, ts.ASPECT)
            out.append([render_sum(rt, c, flags, 3, frames=1) for _, flags in MODES])
        finally:
            c.close()
    for a, b in zip(*out):
        assert a[..., :3].any() and np.array_equal(a, b)

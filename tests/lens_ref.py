"""The thin-lens camera of include/rtx.h (THIN LENS) in numpy: float32, one operation per line of the definition, in the written order.  Fed by the oracle's helpers only:
orc.primary_rays for the pinhole ray (jittered or not), orc.seed_init / orc.tea for the draws, orc.sincos for the angle.  tests/test_lens_ref.py checks that this is a thin
lens; tests/test_lens.py holds the device to it bit for bit."""
import numpy as np

F32 = np.float32
K_TWO_PI = F32(6.28318548202514648)      # kTwoPi, csrc/rtx_math.hpp
JITTER = 2                               # RTX_FLAG_JITTER


def draws(orc, width, height, sample_id, frame_seed, flags):
    """per pixel (row-major): xi1, xi2 of the lens and the seed state after them; the jitter's two draws come first when the flag is set"""
    n = width * height
    xi = np.zeros((n, 2), F32)
    seeds = np.zeros((n, 2), np.uint32)
    for i in range(n):
        s = orc.seed_init(i % width, i // width, sample_id, frame_seed)
        if flags & JITTER:
            _, s = orc.tea(s, 2)
        xi[i], s = orc.tea(s, 2)
        seeds[i] = s
    return xi, seeds


def seeds_without_lens(orc, width, height, sample_id, frame_seed, flags):
    """the seed state a pinhole path starts from: after the jitter's draws only"""
    out = np.zeros((width * height, 2), np.uint32)
    for i in range(width * height):
        s = orc.seed_init(i % width, i // width, sample_id, frame_seed)
        if flags & JITTER:
            _, s = orc.tea(s, 2)
        out[i] = s
    return out


def lens_rays(orc, oracle, params, sample_id, view, radius, focus):
    """oracle: an orc.Oracle whose camera is (view, proj); -> rays8 (H * W, 8) float32 = (o', tmin, d', tmax), seeds (H * W, 2) uint32, and the intermediate
    (o, d, P, cz) of the definition for the property tests"""
    Vi = orc.mat4_inverse(view)
    pin = oracle.primary_rays(params, sample_id)
    o, d = pin[:, 0:3].copy(), pin[:, 4:7].copy()
    xi, seeds = draws(orc, params.width, params.height, sample_id, params.frame_seed, params.flags)
    R, Fd = F32(radius), F32(focus)
    with np.errstate(all="ignore"):
        r = np.sqrt(xi[:, 0])
        sc = np.array([orc.sincos(float(K_TWO_PI * x)) for x in xi[:, 1]], F32).reshape(-1, 2)
        sn, cs = sc[:, 0], sc[:, 1]
        lx = (R * r) * cs
        ly = (R * r) * sn
        cz = np.abs((d[:, 0] * Vi[8] + d[:, 1] * Vi[9]) + d[:, 2] * Vi[10])
        ft = Fd / cz
        P = np.stack([o[:, k] + d[:, k] * ft for k in range(3)], 1)
        ol = np.stack([(o[:, k] + Vi[0 + k] * lx) + Vi[4 + k] * ly for k in range(3)], 1)
        v = P - ol
        r2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        inv = F32(1.0) / np.sqrt(r2)
        dl = v * inv[:, None]
    for a in (r, lx, ly, cz, ft, P, ol, v, r2, inv, dl):
        assert a.dtype == F32
    keep = ~((cz > 0) & np.isfinite(dl).all(1))              # these paths keep the pinhole ray
    rays = pin.copy()
    rays[:, 0:3] = np.where(keep[:, None], o, ol)
    rays[:, 4:7] = np.where(keep[:, None], d, dl)
    return rays, seeds, dict(o=o, d=d, P=P, cz=cz, kept=keep)

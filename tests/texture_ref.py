"""numpy emulation of the diffuse texture maps as include/rtx.h defines them (rtx_set_texture): the two byte -> float tables, Sample, the per-corner UV interpolation at a
hit and Kd' with the package's half_round.  float32 throughout, one numpy operation per written operation (numpy never contracts a multiply and an add).  Shared by
tests/test_texture_ref.py (its own properties, no GPU) and tests/test_texture.py (the device is held to it bit for bit)."""
import math

import numpy as np

F = np.float32


def table(srgb):
    """T[b], b = 0 .. 255: linear (float)b / 255.0f; sRGB decoded in double, rounded to float32 once"""
    if not srgb:
        return np.arange(256, dtype=np.float32) / F(255.0)
    out = np.zeros(256, np.float32)
    for b in range(256):
        c = b / 255.0
        out[b] = F(c / 12.92 if c <= 0.04045 else math.pow((c + 0.055) / 1.055, 2.4))
    return out


def taps(shape, s, t):
    """the four texel coordinates and the two weights of Sample for an image of `shape` (H, W, ...) -> ix0, ix1, iy0, iy1, fx, fy"""
    H, W = shape[:2]
    s, t = np.asarray(s, np.float32), np.asarray(t, np.float32)
    fs, ft = s - np.floor(s), t - np.floor(t)                                  # repeat wrap
    x = fs * F(W) - F(0.5)
    y = (F(1.0) - ft) * F(H) - F(0.5)                                          # OBJ's v runs upward, row 0 is the top
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    return ix % W, (ix + 1) % W, iy % H, (iy + 1) % H, fx, fy                  # (python's % is wrap(i, n) = ((i % n) + n) % n of C)


def sample(rgba8, srgb, s, t):
    """Sample(tex, s, t) -> (n, 3) float32"""
    px = np.asarray(rgba8, np.uint8)
    T = table(srgb)
    ix0, ix1, iy0, iy1, fx, fy = taps(px.shape, s, t)
    out = np.zeros((len(fx), 3), np.float32)
    for k in range(3):
        c00, c10, c01, c11 = T[px[iy0, ix0, k]], T[px[iy0, ix1, k]], T[px[iy1, ix0, k]], T[px[iy1, ix1, k]]
        top = c00 + fx * (c10 - c00)
        bot = c01 + fx * (c11 - c01)
        out[:, k] = top + fy * (bot - top)
    assert out.dtype == np.float32
    return out


def taps_agree(rgba8, s, t):
    """per sample: the four taps read the same r, g, b bytes (Sample then returns T[byte] exactly)"""
    px = np.asarray(rgba8, np.uint8)[..., :3]
    ix0, ix1, iy0, iy1, _, _ = taps(px.shape, s, t)
    a = px[iy0, ix0]
    return np.all((px[iy0, ix1] == a) & (px[iy1, ix0] == a) & (px[iy1, ix1] == a), axis=-1)


def interp_uv(uv3, u, v):
    """texture coordinates at barycentrics (u, v) of triangles whose corner pairs are uv3 (n, 3, 2): s = (b0 * uv0.x + u * uv1.x) + v * uv2.x, t likewise"""
    uv3, u, v = np.asarray(uv3, np.float32), np.asarray(u, np.float32), np.asarray(v, np.float32)
    b0 = F(1.0) - u - v
    s = (b0 * uv3[:, 0, 0] + u * uv3[:, 1, 0]) + v * uv3[:, 2, 0]
    t = (b0 * uv3[:, 0, 1] + u * uv3[:, 1, 1]) + v * uv3[:, 2, 1]
    return s, t


def half_round_array(half_round, x):
    """the package's scalar half_round over an array (each distinct value once)"""
    x = np.asarray(x, np.float32)
    vals, inv = np.unique(x.ravel(), return_inverse=True)
    r = np.array([half_round(float(val)) for val in vals], np.float32)
    return r[inv].reshape(x.shape)


def kd_prime(half_round, kd, tl):
    """Kd'[k] = half_round(m.Kd[k] * tl[k]), m.Kd = half_round(the material's Kd) (the MaterialOptimized table).  kd: (3,) or (n, 3); tl: (n, 3)"""
    table_kd = half_round_array(half_round, np.asarray(kd, np.float32))
    return half_round_array(half_round, table_kd * np.asarray(tl, np.float32))


def pack_rgb8(rgb):
    """debug layers: saturate, v * 255 + 0.5 truncated, alpha 255 -> (n, 4) uint8"""
    c = np.clip(np.asarray(rgb, np.float32), F(0.0), F(1.0))
    out = np.full((len(c), 4), 255, np.uint8)
    out[:, :3] = (c * F(255.0) + F(0.5)).astype(np.int32).astype(np.uint8)
    return out

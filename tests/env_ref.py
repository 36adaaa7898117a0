"""numpy twin of the environment lighting as include/rtx.h defines it (rtx_set_environment): the octahedral mapping both ways, the table builder, the NEAREST lookup, the
importance sampler with its four TEA draws, and the latitude-longitude conversion of the host layer.  The device side is float32, one numpy operation per written operation
(numpy never contracts a multiply and an add); the tables and the conversion are double, summed sequentially (np.cumsum), rounded to float32 once.  Shared by
tests/test_env_ref.py (its own properties, no GPU) and tests/test_env.py (the device is held to it bit for bit)."""
import math

import numpy as np

F = np.float32
EPS = F(0.000001)

# per-sample standard deviation of the one-sample estimator pair (environment NEE + BSDF miss, Lambert plane facing +Y, rho = 0.5) as test_env_ref.py measures it on its two
# inputs with 2^18 samples; that test asserts the measurement still agrees, tests/test_env.py (sun and blocker) sizes its tolerance with SUN_STD
CONST_STD = 0.175
SUN_STD = 10.9


def rot3(m16):
    """R[r][c] = env_to_world[c * 4 + r]; None = identity"""
    if m16 is None:
        return np.eye(3, dtype=np.float32)
    return np.asarray(m16, np.float32).reshape(4, 4).T[:3, :3].copy()


def sgn(x):
    return np.where(x >= 0, F(1.0), F(-1.0)).astype(np.float32)


def from_world(R, d):
    """e = R^T d, each component (R[0][k] * d.x + R[1][k] * d.y) + R[2][k] * d.z"""
    d = np.asarray(d, np.float32)
    return np.stack([(R[0, k] * d[:, 0] + R[1, k] * d[:, 1]) + R[2, k] * d[:, 2] for k in range(3)], axis=1)


def to_world(R, q):
    q = np.asarray(q, np.float32)
    return np.stack([(R[k, 0] * q[:, 0] + R[k, 1] * q[:, 1]) + R[k, 2] * q[:, 2] for k in range(3)], axis=1)


def encode_env(e, n):
    """environment-frame direction -> (u, v, texel j * n + i, r3)"""
    e = np.asarray(e, np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = (np.abs(e[:, 0]) + np.abs(e[:, 1])) + np.abs(e[:, 2])
        qx, qy, qz = e[:, 0] / s, e[:, 1] / s, e[:, 2] / s
        a = np.where(qy >= 0, qx, (F(1.0) - np.abs(qz)) * sgn(qx))
        b = np.where(qy >= 0, qz, (F(1.0) - np.abs(qx)) * sgn(qz))
        u, v = a * F(0.5) + F(0.5), b * F(0.5) + F(0.5)
        i = np.minimum((u * F(n)).astype(np.int64), n - 1)
        j = np.minimum((v * F(n)).astype(np.int64), n - 1)
        r2 = (qx * qx + qy * qy) + qz * qz
        r3 = r2 * np.sqrt(r2)
    for x in (u, v, r3):
        assert x.dtype == np.float32
    return u, v, j * n + i, r3


def decode_env(u, v):
    """(u, v) -> unit direction in the environment frame (n, 3), r3"""
    u, v = np.asarray(u, np.float32), np.asarray(v, np.float32)
    a, b = u * F(2.0) - F(1.0), v * F(2.0) - F(1.0)
    y = (F(1.0) - np.abs(a)) - np.abs(b)
    fa, fb = (F(1.0) - np.abs(b)) * sgn(a), (F(1.0) - np.abs(a)) * sgn(b)
    a, b = np.where(y < 0, fa, a), np.where(y < 0, fb, b)
    r2 = (a * a + y * y) + b * b
    sr = np.sqrt(r2)
    r3 = r2 * sr
    inv = F(1.0) / sr
    q = np.stack([a * inv, y * inv, b * inv], axis=1)
    assert q.dtype == np.float32 and r3.dtype == np.float32
    return q, r3


def centre_r3(n):
    """rc^3 at the texel centres, double, (n, n) indexed [j][i]"""
    c = (np.arange(n, dtype=np.float64) + 0.5) / float(n)
    a, b = np.meshgrid(2.0 * c - 1.0, 2.0 * c - 1.0)            # a varies with i (columns), b with j (rows)
    y = (1.0 - np.abs(a)) - np.abs(b)
    fa, fb = (1.0 - np.abs(b)) * np.where(a >= 0, 1.0, -1.0), (1.0 - np.abs(a)) * np.where(b >= 0, 1.0, -1.0)
    a, b = np.where(y < 0, fa, a), np.where(y < 0, fb, b)
    r2 = (a * a + y * y) + b * b
    return r2 * np.sqrt(r2)


class Tables:
    """what the device holds for a map: texels (n, n, 4) = (r, g, b, pmf), marginal (n,), conditional (n, n); total = the weight sum (double)"""
    def __init__(self, rgb, scale=1.0, to_world_m16=None):
        rgb = np.asarray(rgb, np.float32)
        n = rgb.shape[0]
        assert rgb.shape == (n, n, 3)
        c = rgb * F(scale)                                       # float32 product, once
        assert c.dtype == np.float32
        self.n, self.R = n, rot3(to_world_m16)
        cd = c.astype(np.float64)
        w = (((cd[..., 0] + cd[..., 1]) + cd[..., 2]) / 3.0) / centre_r3(n)
        self.w = w
        self.total = float(np.cumsum(w.ravel())[-1])             # the running sum over all texels, row-major
        self.texels = np.zeros((n, n, 4), np.float32)
        self.texels[..., :3] = c
        self.marginal = np.full(n, 2.0, np.float32)
        self.conditional = np.full((n, n), 2.0, np.float32)
        if not self.total > 0.0:
            return
        self.texels[..., 3] = (w / self.total).astype(np.float32)
        rowacc = np.cumsum(w, axis=1)                            # per row, from 0
        rowsum = rowacc[:, -1]
        acc = np.cumsum(rowsum)
        mass_rows = np.nonzero((w > 0).any(axis=1))[0]
        for j in mass_rows:
            last = np.nonzero(w[j] > 0)[0][-1]
            self.conditional[j, :last] = (rowacc[j, :last] / rowsum[j]).astype(np.float32)
        last_row = mass_rows[-1]
        self.marginal[:last_row] = (acc[:last_row] / self.total).astype(np.float32)

    def pdf(self, pmf, r3):
        out = ((pmf * F(self.n * self.n)) * F(0.25)) * r3
        assert out.dtype == np.float32
        return out

    def eval(self, dirs):
        """world directions (m, 3) -> L (m, 3), pdf, texel, r3"""
        _, _, t, r3 = encode_env(from_world(self.R, dirs), self.n)
        tx = self.texels.reshape(-1, 4)[t]
        return tx[:, :3], self.pdf(tx[:, 3], r3), t, r3

    def sample(self, s0, s1):
        """seeds -> world direction (m, 3), pdf, L (m, 3), texel, s0', s1' after the four draws (row, column, u offset, v offset)"""
        n = self.n
        xr, s0, s1 = tea_next(s0, s1)
        xc, s0, s1 = tea_next(s0, s1)
        xu, s0, s1 = tea_next(s0, s1)
        xv, s0, s1 = tea_next(s0, s1)
        j = search(self.marginal[None, :], xr)
        i = search(self.conditional[j], xc)
        u, v = (i.astype(np.float32) + xu) / F(n), (j.astype(np.float32) + xv) / F(n)
        q, r3 = decode_env(u, v)
        t = j * n + i
        tx = self.texels.reshape(-1, 4)[t]
        return to_world(self.R, q), self.pdf(tx[:, 3], r3), tx[:, :3], t, s0, s1


def search(C, xi):
    """first index with xi < C[index] per row (C: (m, n) or (1, n)); the binary search of the device finds the same on a non-decreasing table, and 0 where there is none"""
    return np.argmax(np.asarray(xi, np.float32)[:, None] < C, axis=1)


def tea_next(s0, s1):
    """RandomFloat (TEA, 4 rounds) on arrays of uint32 seeds -> (float32 in [0, 1], s0', s1')"""
    v0, v1 = np.array(s0, dtype=np.uint32, copy=True), np.array(s1, dtype=np.uint32, copy=True)
    U = np.uint32
    summ = U(0)
    with np.errstate(over="ignore"):
        for _ in range(4):
            summ = U((int(summ) + 0x9e3779b9) & 0xFFFFFFFF)
            v0 = v0 + ((((v1 << U(4)) + U(0xA341316C)) ^ (v1 + summ)) ^ ((v1 >> U(5)) + U(0xC8013EA4)))
            v1 = v1 + ((((v0 << U(4)) + U(0xAD90777D)) ^ (v0 + summ)) ^ ((v0 >> U(5)) + U(0x7E95761E)))
    return v0.astype(np.float32) * F(1.0 / 4294967296.0), v0, v1


# ------------------------------------------------------------------------------------------------
# quadrature on the map's own parametrisation: d_omega = 4 du dv / r^3
# ------------------------------------------------------------------------------------------------
def grid_rows(g, rows):
    """midpoints of a g x g grid, the given rows: environment-frame direction components (x, y, z) and 4 / r^3, double"""
    cu = (np.arange(g, dtype=np.float64) + 0.5) / g
    a, b = np.meshgrid(2.0 * cu - 1.0, 2.0 * cu[rows] - 1.0)
    y = (1.0 - np.abs(a)) - np.abs(b)
    fa, fb = (1.0 - np.abs(b)) * np.where(a >= 0, 1.0, -1.0), (1.0 - np.abs(a)) * np.where(b >= 0, 1.0, -1.0)
    a, b = np.where(y < 0, fa, a), np.where(y < 0, fb, b)
    r = np.sqrt((a * a + y * y) + b * b)
    return a / r, y / r, b / r, 4.0 / (r * r * r)


def solid_angle_sum(g):
    """midpoint sum of 4 / r^3 over the g x g grid: 4 pi"""
    tot = 0.0
    for r0 in range(0, g, 256):
        rows = np.arange(r0, min(g, r0 + 256))
        tot += float(grid_rows(g, rows)[3].sum())
    return tot / (g * g)


def integrate(rgb, g, weight=None):
    """integral over the sphere of map(d) * weight(x, y, z) d_omega, per channel, on a g x g midpoint grid (g a multiple of the map's size); identity rotation"""
    rgb = np.asarray(rgb, np.float64)
    n = rgb.shape[0]
    assert g % n == 0
    k = g // n
    tot = np.zeros(3)
    for r0 in range(0, g, 256):
        rows = np.arange(r0, min(g, r0 + 256))
        x, y, z, w = grid_rows(g, rows)
        if weight is not None:
            w = w * weight(x, y, z)
        tex = rgb[rows // k][:, np.arange(g) // k]
        tot += (tex * w[..., None]).sum(axis=(0, 1))
    return tot / (g * g)


def irradiance_up(rgb, g=4096):
    """E = integral of L(d) max(d.y, 0) d_omega: what a plane facing +Y receives"""
    return integrate(rgb, g, lambda x, y, z: np.maximum(y, 0.0))


def estimator_pair(tab, rho, n, seed):
    """n one-sample estimates of the radiance leaving a Lambert plane (normal +Y, albedo rho) lit by the map alone, as the transport of include/rtx.h forms them: the environment
    NEE sample plus the BSDF-sampled ray's miss, each weighted by the balance heuristic against the other.  Channel 0.  -> (n,) float64"""
    rng = np.random.default_rng(seed)
    s0, s1 = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    d, pdf, L, _, _, _ = tab.sample(s0, s1)
    cos = d[:, 1].astype(np.float64)
    pdf = pdf.astype(np.float64)
    f = rho / math.pi
    ok = (cos >= float(EPS)) & (pdf > 0)
    P = np.where(ok, cos / math.pi, 1.0)
    nee = np.where(ok, L[:, 0] * f * cos / np.where(ok, pdf, 1.0) * (pdf / (pdf + P)), 0.0)
    # cosine-weighted continuation: P = cos / pi, throughput f cos / P = rho
    u1, u2 = rng.random(n), rng.random(n)
    r, phi = np.sqrt(u1), 2.0 * math.pi * u2
    w = np.stack([r * np.cos(phi), np.sqrt(np.maximum(0.0, 1.0 - u1)), r * np.sin(phi)], axis=1).astype(np.float32)
    Lm, pm, _, _ = tab.eval(w)
    Pw = w[:, 1].astype(np.float64) / math.pi
    good = Pw > 0
    miss = np.where(good, Lm[:, 0] * rho * (Pw / (pm.astype(np.float64) + np.where(good, Pw, 1.0))), 0.0)
    return nee + miss


# ------------------------------------------------------------------------------------------------
# the host layer's latitude-longitude conversion (host/ImageIO.h: LatLongToOctahedral), in double
# ------------------------------------------------------------------------------------------------
def sub_samples(W, n):
    return int(min(16.0, max(2.0, math.ceil(W / (2.0 * n)))))


def latlong_lookup(img, x, y, z):
    """nearest texel of a lat-long image (H, W, 3) for unit directions: theta = acos(y) from +Y, phi = atan2(x, -z) in [0, 2 pi)"""
    H, W = img.shape[:2]
    t = np.arccos(np.clip(y, -1.0, 1.0))
    p = np.arctan2(x, -z)
    p = np.where(p < 0.0, p + 2.0 * math.pi, p)
    px = np.clip(np.floor(p / (2.0 * math.pi) * W).astype(np.int64), 0, W - 1)
    py = np.clip(np.floor(t / math.pi * H).astype(np.int64), 0, H - 1)
    return img[py, px]


def latlong_to_octahedral(img, n):
    img = np.asarray(img, np.float32)
    W = img.shape[1]
    S = sub_samples(W, n)
    imgd = img.astype(np.float64)
    out = np.zeros((n, n, 3))
    idx = np.arange(n, dtype=np.float64)
    for sb in range(S):                                           # (b outer, a inner: the order of the sums)
        for sa in range(S):
            u, v = (idx + (sa + 0.5) / S) / n, (idx + (sb + 0.5) / S) / n
            a, b = np.meshgrid(2.0 * u - 1.0, 2.0 * v - 1.0)
            y = (1.0 - np.abs(a)) - np.abs(b)
            fa, fb = (1.0 - np.abs(b)) * np.where(a >= 0, 1.0, -1.0), (1.0 - np.abs(a)) * np.where(b >= 0, 1.0, -1.0)
            a, b = np.where(y < 0, fa, a), np.where(y < 0, fb, b)
            inv = 1.0 / np.sqrt((a * a + y * y) + b * b)
            out += latlong_lookup(imgd, a * inv, y * inv, b * inv)
    return (out / float(S * S)).astype(np.float32)


def latlong_integral(img):
    """integral over the sphere of a lat-long image, per channel: every pixel times its exact solid angle (2 pi / W) (cos t0 - cos t1)"""
    img = np.asarray(img, np.float64)
    H, W = img.shape[:2]
    t = np.arange(H + 1, dtype=np.float64) * math.pi / H
    band = (np.cos(t[:-1]) - np.cos(t[1:])) * (2.0 * math.pi / W)
    return (img * band[:, None, None]).sum(axis=(0, 1))

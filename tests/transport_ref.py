"""transport_ref.py — a float64 numpy twin of the TRANSPORT of rtx_render for the extensions the CPU oracle does not have: diffuse maps, normal maps, alpha cut-outs and
environment lighting, on analytic quads.  It restates the estimator as include/rtx.h (TRANSPORT, PER HIT, NORMAL-MAPPED HIT, HIT RULE, MAPPING) and the HLSL-derived
tests/ggx_ref64.py define it — the same ESTIMATOR, not the same random SEQUENCE (plain numpy.random.Generator streams) — and nothing else: ray / quad intersection in
float64, no BVH, no bias offsets, vectorised over paths.  tests/test_transport_ref.py proves it on the CPU, tests/golden/make_transport_ref.py runs it at full sample
counts into tests/golden/transport_ref.npz, and tests/test_transport.py holds the GPU's converged frames to those expectations.

NOT the textbook integral under GGX: sample_ggx flips a sampled direction that lands below the normal instead of rejecting it, and the continuation weight uses the
unclamped NdotL (Sampler_v6.hlsl:455), so the expectation of the estimator is not the integral of f L cos.  The twin restates both; test_transport_ref.py reports the gap.

OUT OF SCOPE: RTX_FLAG_TRANSMISSION, the thin lens, RTX_FLAG_JITTER, Russian roulette (the tests keep rr_start >= max_bounces), RTX_ENV_HIDDEN.

Per bounce, in the order of shade_item: the nee_samples triangle-light samples (CDF pick, xi1, xi2 with the fold, pdf_light, mi = pdf_light / (nee pdf_light + P)), the one
environment sample (four draws, mi = pdf_env / (pdf_env + P), rejected when cos_x < EPS), the continuation (select_strategy, sample_ggx / sample_lambert,
thr *= F NdotL / P with the unclamped NdotL, stop on not P > 0).  Emitter hit at bounce >= 1: mi = prev_pdf / (nee pdf_light + prev_pdf).  Miss at bounce >= 1:
mi = prev_pdf / (pdf_env(d) + prev_pdf); at bounce 0 it adds L(d).

THE ONE PLACE WHERE AN OFFSET DECIDES SOMETHING.  A shadow ray starts at pos + kSBias n' with tmin = kSBias / 2, a continuation ray at pos itself with tmin = kSBias.  Away
from edges that makes no difference except for a direction that leaves towards the FAR side of the shading point's own quad (possible once n' differs from the geometric
normal): the shadow ray then crosses its own quad at t = kSBias cos(n', n) / |d . n| > kSBias / 2 and is occluded, the continuation ray starts on the quad and passes.
The twin states exactly that: a shadow segment that leaves to the far side of its own quad is blocked, a continuation ray never sees its own quad.

WHAT THE TWIN DOES NOT SHARE WITH FLOAT32.  The continuation ray starts at the float32 hit position, which lies up to about 3e-7 off its quad's plane, with tmin = kSBias =
2e-5: a direction within about 0.01 of the plane can re-hit the quad it starts on (from behind when the position fell below), which exact arithmetic never does.  Replaying
the device's own random numbers through the twin (radiance(draws=...)) reproduces the device's one-sample frames to 1e-6 per sample except for these paths, about one in a
thousand; their effect on a block mean was measured at up to 1.4 standard errors of the fixture (0.05 % of the mean) — inside the six the GPU test allows, and recorded in
profiles/transport_energy.md.  It is the reference's own bias scheme in float32 (un-offset origin, Sampler_v6.hlsl:224-227), on mapped and unmapped surfaces alike.

wrong= selects exactly one deliberate error (WRONG); these exist for the power check of test_transport_ref.py and never run on a GPU.
"""
import hashlib

import numpy as np

import env_ref as er
import ggx_ref64 as R
import normalmap_ref as nr
import texture_ref as tr

PI, EPS = R.PI, R.EPSILON
LAMBERT_ONLY = 1
T_MAX = 10000.0
F999 = float(np.float32(0.999))
TWO_PI_LAMBERT = 2.0 * 3.14159265358979                       # Lambertian_v6.hlsl:10; the GGX sampler uses 2 * PI with PI = 3.1415f

WRONG = ("n_geometric_in_nee", "n_geometric_in_continuation", "n_geometric_in_view_terms",
         "kd_untextured_in_env_nee", "kd_untextured_in_light_nee", "kd_untextured_in_continuation",
         "no_mis_env_nee", "no_mis_env_miss", "r3_of_texel_centre", "texture_nearest", "green_flipped", "handedness_ignored",
         "cutout_ignored_by_shadow_rays", "cutout_ignored_by_closest_hit", "env_rotation_transposed")


def _dot(a, b):
    return (a * b).sum(-1)


def _unit(v):
    return v / np.sqrt(_dot(v, v))[..., None]


# ------------------------------------------------------------------------------------------------
# vectorised forms of ggx_ref64's scalar samplers, and the mixture with the view terms on a normal of their own
# ------------------------------------------------------------------------------------------------
def coordinate_system_v(N):
    """GGX_v6.hlsl:65-76 for N (k, 3)"""
    z = np.abs(N[:, 2]) < F999
    ax = np.where(z[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    T = _unit(np.cross(ax, N))
    return T, np.cross(N, T)


def sample_ggx_v(Pr, outgoing, normal, U1, U2):
    """SampleBRDF_GGX, GGX_v6.hlsl:93-169 -> the sampled direction (flipped, not rejected, when it lands below the normal)"""
    alpha = Pr * Pr
    N, V = _unit(normal), _unit(outgoing)
    T1, T2 = coordinate_system_v(N)
    Ve = _unit(np.stack([alpha * _dot(T1, V), alpha * _dot(T2, V), _dot(N, V)], -1))
    lensq = Ve[:, 0] * Ve[:, 0] + Ve[:, 1] * Ve[:, 1]
    pos = lensq > 0.0
    rs = np.sqrt(np.where(pos, lensq, 1.0))
    T1h = np.where(pos[:, None], np.stack([-Ve[:, 1], Ve[:, 0], np.zeros_like(lensq)], -1) / rs[:, None], np.array([1.0, 0.0, 0.0]))
    T2h = np.cross(Ve, T1h)
    r = np.sqrt(U1)
    phi = 2.0 * PI * U2
    t1, t2 = r * np.cos(phi), r * np.sin(phi)
    s = 0.5 * (1.0 + Ve[:, 2])
    t2 = (1.0 - s) * np.sqrt(R.saturate(1.0 - t1 * t1)) + s * t2
    Nh = t1[:, None] * T1h + t2[:, None] * T2h + np.sqrt(R.saturate(1.0 - t1 * t1 - t2 * t2))[:, None] * Ve
    Ne = _unit(np.stack([alpha * Nh[:, 0], alpha * Nh[:, 1], np.maximum(0.0, Nh[:, 2])], -1))
    H = Ne[:, 0:1] * T1 + Ne[:, 1:2] * T2 + Ne[:, 2:3] * N
    I = -V
    smp = I - 2.0 * _dot(H, I)[:, None] * H
    return np.where((_dot(smp, normal) < 0.0)[:, None], -smp, smp)


def sample_lambert_v(normal, u1, u2):
    """SampleBRDF_Lambertian, Lambertian_v6.hlsl:2-38"""
    r = np.sqrt(u1)
    theta = TWO_PI_LAMBERT * u2
    x, y = r * np.cos(theta), r * np.sin(theta)
    z = np.sqrt(np.maximum(0.0, 1.0 - x * x - y * y))
    up = np.where((np.abs(normal[:, 2]) < F999)[:, None], np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    right = _unit(np.cross(up, normal))
    fwd = np.cross(normal, right)
    s = _unit(x[:, None] * right + y[:, None] * fwd + z[:, None] * normal)
    return np.where((_dot(s, normal) < 0.0)[:, None], -s, s)


def mixture_v(m, normal, L, V, kdpi, lambert, n_view=None):
    """F = p_d f_lambert + p_s f_ggx, P = p_d pdf_lambert + p_s pdf_ggx as ggx_ref64.mixture forms them, over (k, 3) arrays, with kdpi (k, 3) or (3,) as the Lambert
    term (Kd' / PI under a map) and — for the wrong variant that needs it — the VIEW terms of the mixture (strategy probabilities, N.V, G1(V), Ess: mix_view) taken on
    n_view instead of normal.  n_view None: exactly ggx_ref64.mixture's operations."""
    q0 = np.maximum(_dot(normal, L), EPS) / PI
    if lambert:
        return np.broadcast_to(kdpi, L.shape).copy(), q0
    nv = normal if n_view is None else n_view
    pd, ps = R.strategy_probs(m, V, nv)
    N, Nv, Vn, Ln = _unit(normal), _unit(nv), _unit(V), _unit(L)
    H = _unit(Vn + Ln)
    NdotV, NdotL, NdotH, VdotH = _dot(Nv, Vn), _dot(N, Ln), _dot(N, H), _dot(Vn, H)
    Fr = R.schlick(m.Ks, VdotH)
    D = R.d_ggx(NdotH, m.Pr)
    G = R.g2_smith(NdotV, NdotL, m.Pr * m.Pr)
    den = 4.0 * NdotV * NdotL
    with np.errstate(divide="ignore", invalid="ignore"):
        spec = Fr * (D * G / den)[:, None]
        Ess = R.ess_lut(m, NdotV)
        kms = (1.0 - Ess) / Ess
        f1 = spec * (1.0 + m.Ks * kms[:, None])
        q1 = R.g1_smith(NdotV, m.Pr * m.Pr) * D / (NdotV * 4.0)
    bad = (den < EPS) | ~np.isfinite(f1).all(-1)
    f1 = np.where(bad[:, None], 0.0, f1)
    return pd[:, None] * kdpi + ps[:, None] * f1, pd * q0 + ps * q1


# ------------------------------------------------------------------------------------------------
# maps, in float64 from the rtx.h text
# ------------------------------------------------------------------------------------------------
def sample_image(img, s, t, nearest=False):
    """Sample(): bilinear with repeat wrap over img (H, W, C) float64 (texels already through their byte -> float table); nearest: the texel the point lies in"""
    H, W = img.shape[:2]
    fs, ft = s - np.floor(s), t - np.floor(t)
    x, y = fs * W - 0.5, (1.0 - ft) * H - 0.5
    if nearest:
        ix, iy = np.floor(x + 0.5).astype(np.int64) % W, np.floor(y + 0.5).astype(np.int64) % H
        return img[iy, ix]
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    ix, iy = x0.astype(np.int64), y0.astype(np.int64)
    ix0, ix1, iy0, iy1 = ix % W, (ix + 1) % W, iy % H, (iy + 1) % H
    top = img[iy0, ix0] + fx * (img[iy0, ix1] - img[iy0, ix0])
    bot = img[iy1, ix0] + fx * (img[iy1, ix1] - img[iy1, ix0])
    return top + fy * (bot - top)


def kd_prime(kd_table, tl):
    """Kd'[k] = half_round(m.Kd[k] * tl[k]) with m.Kd the binary16-rounded table value"""
    return R.half(kd_table * tl)


def perturb_v(n, Tw, Bw, c, wo, green_flipped=False, handedness_ignored=False):
    """NORMAL-MAPPED HIT: n (3,) the quad's world shading normal, Tw / Bw (3,) the world tangent / bitangent of the triangle record, c (k, 3) decoded texels,
    wo (k, 3) -> n' (k, 3)"""
    k = len(c)
    out = np.broadcast_to(n, (k, 3)).copy()
    tv = Tw - n * _dot(n, Tw)
    l2 = _dot(tv, tv)
    if not (l2 > 0.0) or np.isinf(l2):
        return out
    t = tv / np.sqrt(l2)
    bv = np.cross(n, t)
    sg = -1.0 if (_dot(bv, Bw) < 0.0 and not handedness_ignored) else 1.0
    cy = -c[:, 1:2] if green_flipped else c[:, 1:2]
    m = (t * c[:, 0:1] + (bv * sg) * cy) + n * c[:, 2:3]
    m2 = _dot(m, m)
    with np.errstate(all="ignore"):
        npr = m / np.sqrt(m2)[:, None]
    a, ap = wo @ n, _dot(npr, wo)
    flat = (c[:, 0] == 0.0) & (c[:, 1] == 0.0)
    guard = ((a > 0) & ~(ap > 0)) | ((a < 0) & ~(ap < 0))
    use = ~flat & (m2 > 0.0) & np.isfinite(m2) & ~guard
    out[use] = npr[use]
    return out


class Env:
    """the octahedral map in float64 (MAPPING): pmf, CDFs and texels are env_ref.Tables' float32 values cast up"""
    def __init__(self, img, to_world=None, scale=1.0, transposed=False, centre_r3=False):
        tab = er.Tables(img, scale, to_world)
        self.n = tab.n
        self.R = tab.R.astype(np.float64)
        if transposed:
            self.R = self.R.T.copy()
        self.L = tab.texels[..., :3].astype(np.float64).reshape(-1, 3)
        self.pmf = tab.texels[..., 3].astype(np.float64).ravel()
        self.marginal, self.conditional = tab.marginal.astype(np.float64), tab.conditional.astype(np.float64)
        self.rc3 = er.centre_r3(self.n).ravel() if centre_r3 else None

    def pdf_of(self, t, r3):
        if self.rc3 is not None:
            r3 = self.rc3[t]
        return ((self.pmf[t] * float(self.n * self.n)) * 0.25) * r3

    def eval(self, d):
        """world directions (k, 3) -> L (k, 3), pdf (k,)"""
        n = self.n
        e = d @ self.R                                           # e = R^T d
        s = np.abs(e).sum(-1)
        q = e / s[:, None]
        sx, sz = np.where(q[:, 0] >= 0, 1.0, -1.0), np.where(q[:, 2] >= 0, 1.0, -1.0)
        up = q[:, 1] >= 0
        a = np.where(up, q[:, 0], (1.0 - np.abs(q[:, 2])) * sx)
        b = np.where(up, q[:, 2], (1.0 - np.abs(q[:, 0])) * sz)
        u, v = a * 0.5 + 0.5, b * 0.5 + 0.5
        i, j = np.minimum((u * n).astype(np.int64), n - 1), np.minimum((v * n).astype(np.int64), n - 1)
        t = j * n + i
        r2 = _dot(q, q)
        return self.L[t], self.pdf_of(t, r2 * np.sqrt(r2))

    def decode(self, u, v):
        """(u, v) -> world direction (k, 3), r3"""
        a, b = u * 2.0 - 1.0, v * 2.0 - 1.0
        y = (1.0 - np.abs(a)) - np.abs(b)
        fa, fb = (1.0 - np.abs(b)) * np.where(a >= 0, 1.0, -1.0), (1.0 - np.abs(a)) * np.where(b >= 0, 1.0, -1.0)
        a, b = np.where(y < 0, fa, a), np.where(y < 0, fb, b)
        r2 = (a * a + y * y) + b * b
        sr = np.sqrt(r2)
        q = np.stack([a, y, b], -1) / sr[:, None]
        return q @ self.R.T, r2 * sr                             # d = R q

    def sample(self, xr, xc, xu, xv):
        """the four draws (row, column, u offset, v offset) -> direction, pdf, L; selection = first index with xi < C[index]"""
        n = self.n
        j = np.minimum(np.searchsorted(self.marginal, xr, side="right"), n - 1)
        i = np.minimum((xc[:, None] >= self.conditional[j]).sum(1), n - 1)
        d, r3 = self.decode((i + xu) / n, (j + xv) / n)
        t = j * n + i
        return d, self.pdf_of(t, r3), self.L[t]


# ------------------------------------------------------------------------------------------------
# the scene as analytic quads
# ------------------------------------------------------------------------------------------------
class Quad:
    pass


def scene_hash(scene):
    """sha256 over every array the renderer and the twin read"""
    h = hashlib.sha256()

    def put(a, dt):
        a = np.ascontiguousarray(a, dtype=dt)
        h.update(str(a.shape).encode()); h.update(a.tobytes())
    put(scene.materials, np.float32)
    for (v, i, m), uv in zip(scene.meshes, scene.uvs):
        put(v, np.float32); put(i, np.uint32); put(m, np.uint32); put(uv, np.float32)
    for mesh, o2w in scene.instances:
        put([mesh], np.uint32); put(o2w, np.float32)
    for px, srgb in scene.textures:
        put(px, np.uint8); put([int(srgb)], np.uint32)
    for maps in (scene.material_maps, scene.opacity_maps, scene.normal_maps):
        put([-1 if t is None else t for t in maps], np.int32)
    env = scene.environment
    if env is not None:
        put(env["img"], np.float32); put(env["to_world"], np.float32); put([env["scale"]], np.float32)
    for m in scene.view_proj(scene.aspect):
        put(m, np.float32)
    put([scene.nee_samples, scene.width, scene.height], np.uint32)
    return h.hexdigest()


def quads_of(scene):
    """every mesh is a list of quads: vertices 4 q .. 4 q + 3 (a parallelogram v0, v1, v2 = v1 + v3 - v0, v3), index entries (0, 1, 2, 0, 2, 3), one material, one vertex
    normal; UVs per index entry.  -> [Quad] in world space, float64 from the float32 arrays"""
    mats = np.asarray(scene.materials, np.float32).reshape(-1, 32)
    out = []
    for mesh, o2w in scene.instances:
        v, idx, mid = scene.meshes[mesh]
        v = np.asarray(v, np.float32).astype(np.float64).reshape(-1, 7)
        uv = np.asarray(scene.uvs[mesh], np.float32).reshape(-1, 2)
        M16 = np.asarray(o2w, np.float32).astype(np.float64).reshape(16)
        M = M16.reshape(4, 4).T                                   # column-vector matrix: element (r, c) at m[c * 4 + r]
        nrm = np.linalg.inv(M[:3, :3]).T
        for q in range(len(idx) // 6):
            ii = np.asarray(idx[6 * q:6 * q + 6], np.int64)
            assert (ii == ii[0] + np.array([0, 1, 2, 0, 2, 3])).all() and len(set(np.asarray(mid[6 * q:6 * q + 6]).tolist())) == 1
            po = v[ii[0]:ii[0] + 4, :3]
            pw = po @ M[:3, :3].T + M[:3, 3]
            Q = Quad()
            Q.P0, Q.E1, Q.E2 = pw[0], pw[1] - pw[0], pw[3] - pw[0]
            assert np.abs(pw[2] - (pw[1] + pw[3] - pw[0])).max() < 1e-5
            g11, g12, g22 = Q.E1 @ Q.E1, Q.E1 @ Q.E2, Q.E2 @ Q.E2
            det = g11 * g22 - g12 * g12
            Q.D1, Q.D2 = (g22 * Q.E1 - g12 * Q.E2) / det, (g11 * Q.E2 - g12 * Q.E1) / det
            Q.area = float(np.linalg.norm(np.cross(Q.E1, Q.E2)))
            Q.N = _unit(nrm @ v[ii[0], 3:6])                      # the world shading normal (Hit_v6.hlsl:56); all four vertex normals are equal
            assert abs(abs(Q.N @ _unit(np.cross(Q.E1, Q.E2))) - 1.0) < 1e-5
            Q.mat = int(mid[6 * q])
            m = mats[Q.mat]
            Q.m = R.Mat(m[0:3], m[4:7], m[12], m[13], m[16:32])
            Q.Ke = R.half(m[8:11])
            Q.emits = bool((m[8:11] > 0).any())
            Q.M16 = M16
            Q.uv3 = uv[6 * q:6 * q + 6].reshape(2, 3, 2).astype(np.float64)
            p3 = np.stack([po[[0, 1, 2]], po[[0, 2, 3]]]).astype(np.float32)
            Q.tan6 = nr.tangent_records(p3, uv[6 * q:6 * q + 6].reshape(2, 3, 2)).astype(np.float64)
            M3 = M[:3, :3]
            Q.Tw, Q.Bw = Q.tan6[:, :3] @ M3.T, Q.tan6[:, 3:] @ M3.T
            tex = lambda maps: -1 if (Q.emits or maps is None or Q.mat >= len(maps) or maps[Q.mat] is None) else int(maps[Q.mat])
            Q.kd_tex, Q.cut_tex, Q.nrm_tex = tex(scene.material_maps), tex(scene.opacity_maps), tex(scene.normal_maps)
            out.append(Q)
    return out


class Twin:
    def __init__(self, scene, flags=0, wrong=None):
        assert wrong is None or wrong in WRONG
        self.wrong, self.lambert = wrong, bool(flags & LAMBERT_ONLY)
        self.quads = quads_of(scene)
        self.nee = int(scene.nee_samples)
        self.kd_img, self.nrm_img, self.alpha_img = {}, {}, {}
        Nt = nr.table().astype(np.float64)
        for k, (px, srgb) in enumerate(scene.textures):
            px = np.asarray(px, np.uint8)
            self.kd_img[k] = tr.table(srgb).astype(np.float64)[px[..., :3]]
            self.nrm_img[k] = Nt[px[..., :3]]
            self.alpha_img[k] = tr.table(False).astype(np.float64)[px[..., 3:4]]
        env = scene.environment
        self.env = None if env is None else Env(env["img"], env["to_world"], env["scale"], transposed=wrong == "env_rotation_transposed", centre_r3=wrong == "r3_of_texel_centre")
        # the light list: emissive triangles, weight = area * mean(Ke), pdf_l = (weight / total) / area (SampleLightNEE_GI)
        self.lights = [(qi, tri) for qi, Q in enumerate(self.quads) if Q.emits for tri in range(2)]
        if not self.lights:
            self.nee = 0
        w = np.array([0.5 * self.quads[qi].area * float(self.quads[qi].Ke.mean()) for qi, _ in self.lights])
        self.total_weight = float(w.sum()) if len(w) else 0.0
        self.cdf = np.cumsum(w) / self.total_weight if len(w) else w

    # ---- geometry ----
    def uv_at(self, Q, a, b):
        """per-corner UV interpolation on the triangle the point lies in: triangle 0 = (v0, v1, v2) where a >= b, u = a - b, v = b; triangle 1 = (v0, v2, v3), u = a, v = b - a"""
        tri = (a < b).astype(np.int64)
        u, v = np.where(tri == 0, a - b, a), np.where(tri == 0, b, b - a)
        uv3 = Q.uv3[tri]
        st = (1.0 - u - v)[:, None] * uv3[:, 0] + u[:, None] * uv3[:, 1] + v[:, None] * uv3[:, 2]
        return st[:, 0], st[:, 1], tri

    def alpha_ok(self, Q, a, b):
        s, t, _ = self.uv_at(Q, a, b)
        return sample_image(self.alpha_img[Q.cut_tex], s, t)[:, 0] >= 0.5

    def _cross(self, Q, o, d):
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((Q.P0 - o) @ Q.N) / (d @ Q.N)
            x = o + t[:, None] * d - Q.P0
            a, b = x @ Q.D1, x @ Q.D2
        return t, a, b, np.isfinite(t) & (t > 0.0) & (a >= 0.0) & (a <= 1.0) & (b >= 0.0) & (b <= 1.0)

    def closest(self, o, d, skip):
        """-> quad index (-1 = miss), t, a, b; `skip` (k,) = the quad the ray starts on"""
        k = len(o)
        best, bq, ba, bb = np.full(k, np.inf), np.full(k, -1, np.int64), np.zeros(k), np.zeros(k)
        for qi, Q in enumerate(self.quads):
            t, a, b, ok = self._cross(Q, o, d)
            ok &= (skip != qi) & (t < best)
            if Q.cut_tex >= 0 and self.wrong != "cutout_ignored_by_closest_hit" and ok.any():
                sel = np.nonzero(ok)[0]
                ok[sel] = self.alpha_ok(Q, a[sel], b[sel])
            best, bq, ba, bb = np.where(ok, t, best), np.where(ok, qi, bq), np.where(ok, a, ba), np.where(ok, b, bb)
        return bq, best, ba, bb

    def visible(self, own, side, o, d, tmax, target=-1):
        """an exact segment (o, o + tmax d) against every quad but `target`; the own quad blocks a direction that leaves to its far side (module docstring);
        side (k,) = the sign of n' . N of the own quad"""
        vis = np.ones(len(o), bool)
        for qi, Q in enumerate(self.quads):
            if qi == target:
                continue
            if qi == own:
                vis &= ~((d @ Q.N) * side < 0.0)
                continue
            t, a, b, ok = self._cross(Q, o, d)
            ok &= t < tmax
            if Q.cut_tex >= 0 and self.wrong != "cutout_ignored_by_shadow_rays" and ok.any():
                sel = np.nonzero(ok)[0]
                ok[sel] = self.alpha_ok(Q, a[sel], b[sel])
            vis &= ~ok
        return vis

    # ---- the shading point ----
    def surface(self, Q, a, b, wo):
        """-> Kd' / PI (k, 3), the material's Kd / PI (3,), n' (k, 3)"""
        k = len(a)
        plain = Q.m.Kd[:3] / PI
        s, t, tri = self.uv_at(Q, a, b)
        near = self.wrong == "texture_nearest"
        kdpi = np.broadcast_to(plain, (k, 3))
        if Q.kd_tex >= 0:
            kdpi = kd_prime(Q.m.Kd[:3], sample_image(self.kd_img[Q.kd_tex], s, t, near)) / PI
        n = np.broadcast_to(Q.N, (k, 3)).copy()
        if Q.nrm_tex >= 0:
            c = sample_image(self.nrm_img[Q.nrm_tex], s, t, near)
            for tr_ in range(2):
                sel = tri == tr_
                if sel.any():
                    n[sel] = perturb_v(Q.N, Q.Tw[tr_], Q.Bw[tr_], c[sel], wo[sel], self.wrong == "green_flipped", self.wrong == "handedness_ignored")
        return kdpi, plain, n

    def light_pdf_area(self, qi):
        Q = self.quads[qi]
        return (float(Q.Ke.mean()) / self.total_weight)           # pdf_l: per unit area

    # ---- one batch of paths ----
    def radiance(self, o, d, max_bounces, rng, draws=None):
        """o, d (k, 3) primary rays -> (max_bounces, k, 3): entry m - 1 = the estimate of one sample with max_bounces = m (a path of m segments is a prefix of a longer one:
        the last bounce still casts its NEE samples and only skips the continuation).  Every path draws 10 numbers per bounce whatever happens to it, so that two runs
        with the same generator (right and wrong) use common random numbers.  draws (optional): per bounce a (k, 10) array used instead of the generator — columns 0-2
        the light sample (pick, xi1, xi2), 3-6 the environment sample (row, column, u, v), 7 the strategy draw, 8-9 the BSDF sample — e.g. a device sequence."""
        k = len(o)
        w = self.wrong
        rad = np.zeros((k, 3))
        out = np.zeros((max_bounces, k, 3))
        thr = np.ones((k, 3))
        prev = np.ones(k)
        alive = np.ones(k, bool)
        skip = np.full(k, -1, np.int64)
        o, d = np.array(o, np.float64), np.array(d, np.float64)
        for bounce in range(max_bounces):
            xi = rng.random((k, 10)) if draws is None else draws[bounce]
            hq, ht, ha, hb = self.closest(o, d, skip)
            hq = np.where(alive, hq, -2)
            # the ray left the scene
            miss = np.nonzero(hq == -1)[0]
            if self.env is not None and len(miss):
                L, pdf = self.env.eval(d[miss])
                if bounce == 0:
                    rad[miss] += L
                else:
                    mi = np.ones(len(miss)) if w == "no_mis_env_miss" else prev[miss] / (pdf + prev[miss])
                    e = (L * thr[miss]) * mi[:, None]
                    rad[miss] += np.where(np.isfinite(e).all(-1)[:, None], e, 0.0)
            nxt_alive = np.zeros(k, bool)
            no, nd, nthr, nprev, nskip = o.copy(), d.copy(), thr.copy(), prev.copy(), skip.copy()
            for qi, Q in enumerate(self.quads):
                sel = np.nonzero(hq == qi)[0]
                if not len(sel):
                    continue
                pos = o[sel] + ht[sel, None] * d[sel]
                if Q.emits:                                       # Hit.hlsl:126-174
                    if bounce == 0:
                        rad[sel] += Q.Ke
                    else:
                        mi = np.ones(len(sel))
                        if self.nee:
                            Lv = pos - o[sel]
                            dist2 = _dot(Lv, Lv)
                            cos_t = np.abs(-d[sel] @ Q.N)
                            pdf_light = self.light_pdf_area(qi) * dist2 / np.maximum(cos_t, EPS)
                            mi = prev[sel] / (self.nee * pdf_light + prev[sel])
                        e = Q.Ke * thr[sel] * mi[:, None]
                        rad[sel] += np.where(np.isfinite(e).all(-1)[:, None], e, 0.0)
                    continue
                wo = -d[sel]
                kdpi, plain, n = self.surface(Q, ha[sel], hb[sel], wo)
                ngeo = np.broadcast_to(Q.N, n.shape)
                side = np.where(n @ Q.N < 0.0, -1.0, 1.0)
                n_view = ngeo if w == "n_geometric_in_view_terms" else None
                n_nee = ngeo if w == "n_geometric_in_nee" else n
                x = xi[sel]
                T = thr[sel]
                # triangle-light samples
                for j in range(self.nee):
                    assert self.nee == 1, "one draw triple per bounce is provided"
                    li = np.minimum(np.searchsorted(self.cdf, x[:, 0], side="right"), len(self.lights) - 1)
                    xi1, xi2 = x[:, 1].copy(), x[:, 2].copy()
                    fold = xi1 + xi2 > 1.0
                    xi1, xi2 = np.where(fold, 1.0 - xi1, xi1), np.where(fold, 1.0 - xi2, xi2)
                    con = np.zeros((len(sel), 3))
                    for l, (lq, ltri) in enumerate(self.lights):
                        ls = np.nonzero(li == l)[0]
                        if not len(ls):
                            continue
                        E = self.quads[lq]
                        xv, yv, zv = (E.P0, E.P0 + E.E1, E.P0 + E.E1 + E.E2) if ltri == 0 else (E.P0, E.P0 + E.E1 + E.E2, E.P0 + E.E2)
                        sp = (1.0 - xi1[ls] - xi2[ls])[:, None] * xv + xi1[ls, None] * yv + xi2[ls, None] * zv
                        Lv = sp - pos[ls]
                        dist2 = _dot(Lv, Lv)
                        dist = np.sqrt(dist2)
                        Ln = Lv / dist[:, None]
                        cos_x, cos_y = _dot(n_nee[ls], Ln), np.abs(Ln @ E.N)
                        ok = ~((cos_x < EPS) | (cos_y < EPS))
                        pdf_light = self.light_pdf_area(lq) * dist2 / np.where(ok, cos_y, 1.0)
                        kd = plain if w == "kd_untextured_in_light_nee" else kdpi[ls]
                        F, P = mixture_v(Q.m, n_nee[ls], Ln, wo[ls], kd, self.lambert, None if n_view is None else n_view[ls])
                        with np.errstate(all="ignore"):
                            mi = pdf_light / (self.nee * pdf_light + P)
                            c = E.Ke * (T[ls] * F) * (cos_x / pdf_light * mi)[:, None]
                        ok &= np.isfinite(c).all(-1)
                        ok[ok] = self.visible(qi, side[ls][ok], pos[ls][ok], Ln[ok], dist[ok], target=lq)
                        con[ls] = np.where(ok[:, None], c, 0.0)
                    rad[sel] += con
                # the environment's sample
                if self.env is not None:
                    Ln, pdf, L = self.env.sample(x[:, 3], x[:, 4], x[:, 5], x[:, 6])
                    cos_x = _dot(n_nee, Ln)
                    ok = ~(cos_x < EPS) & (pdf > 0.0)
                    kd = plain if w == "kd_untextured_in_env_nee" else kdpi
                    F, P = mixture_v(Q.m, n_nee, Ln, wo, kd, self.lambert, n_view)
                    with np.errstate(all="ignore"):
                        mi = np.ones(len(sel)) if w == "no_mis_env_nee" else pdf / (pdf + P)
                        c = L * (T * F) * (cos_x / pdf * mi)[:, None]
                    ok &= np.isfinite(c).all(-1) & (c != 0.0).any(-1)
                    ok[ok] = self.visible(qi, side[ok], pos[ok], Ln[ok], T_MAX)
                    rad[sel] += np.where(ok[:, None], c, 0.0)
                # the continuation
                if bounce + 1 < max_bounces:
                    n_c = ngeo if w == "n_geometric_in_continuation" else n
                    nvc = n_c if n_view is None else n_view
                    if self.lambert:
                        smp = sample_lambert_v(n_c, x[:, 8], x[:, 9])
                    else:
                        _, ps = R.strategy_probs(Q.m, wo, nvc)
                        ggx = (x[:, 7] <= ps) & (Q.m.Pr >= 0.04)
                        smp = np.where(ggx[:, None], sample_ggx_v(Q.m.Pr, wo, n_c, x[:, 8], x[:, 9]), sample_lambert_v(n_c, x[:, 8], x[:, 9]))
                    kd = plain if w == "kd_untextured_in_continuation" else kdpi
                    F, P = mixture_v(Q.m, n_c, smp, wo, kd, self.lambert, n_view)
                    NdotL = _dot(n_c, smp)                        # unclamped, Sampler_v6.hlsl:455
                    with np.errstate(all="ignore"):
                        T2 = T * (F * (NdotL / P)[:, None])
                    go = (P > 0.0) & np.isfinite(T2).all(-1) & (T2 != 0.0).any(-1)
                    g = sel[go]
                    nxt_alive[g] = True
                    no[g], nd[g], nthr[g], nprev[g], nskip[g] = pos[go], smp[go], T2[go], P[go], qi
            out[bounce] = rad
            alive, o, d, thr, prev, skip = nxt_alive, no, nd, nthr, nprev, nskip
        return out


# ------------------------------------------------------------------------------------------------
# the deterministic expectations
# ------------------------------------------------------------------------------------------------
def _primary_points(tw, o, d):
    hq, ht, ha, hb = tw.closest(o, d, np.full(len(o), -1, np.int64))
    return hq, o + np.where(np.isfinite(ht), ht, 0.0)[:, None] * d, ha, hb


def nee_only_expectation(tw, o, d, g_env=64, g_light=48):
    """max_bounces = 1: bounce 0's own term (emitter hit: Ke, miss: L(d)) plus the expectation of the NEE samples of the primary hit, noise-free:
    over the environment the integral of L F cos pdf_env / (pdf_env + P) V on a g_env^2 midpoint grid of the octahedral square (d_omega = 4 du dv / r^3), over the
    emitter's area the integral of Ke F cos_x cos_y / dist^2 mi V on g_light^2 midpoints per emitter quad.  -> (k, 3)"""
    k = len(o)
    out = np.zeros((k, 3))
    hq, pos, ha, hb = _primary_points(tw, o, d)
    if tw.env is not None:
        m = np.nonzero(hq == -1)[0]
        if len(m):
            out[m] = tw.env.eval(d[m])[0]
        c = (np.arange(g_env) + 0.5) / g_env
        U, V = (a.ravel() for a in np.meshgrid(c, c))
        Ldir, r3 = tw.env.decode(U, V)
        Lrad, pdf_env = tw.env.eval(Ldir)
        dom = 4.0 / r3 / (g_env * g_env)
        lit = np.nonzero((Lrad.sum(-1) > 0.0) & (pdf_env > 0.0))[0]
        Ldir, Lrad, pdf_env, dom = Ldir[lit], Lrad[lit], pdf_env[lit], dom[lit]
    for qi, Q in enumerate(tw.quads):
        sel = np.nonzero(hq == qi)[0]
        if not len(sel):
            continue
        if Q.emits:
            out[sel] += Q.Ke
            continue
        wo = -d[sel]
        kdpi, plain, n = tw.surface(Q, ha[sel], hb[sel], wo)
        side = np.where(n @ Q.N < 0.0, -1.0, 1.0)
        for p_, p in enumerate(sel):                              # one shading point at a time, all directions at once
            one = lambda a, cnt: np.broadcast_to(a, (cnt,) + np.shape(a))
            if tw.env is not None:
                G = len(Ldir)
                cos_x = Ldir @ n[p_]
                F, P = mixture_v(Q.m, one(n[p_], G), Ldir, one(wo[p_], G), kdpi[p_], tw.lambert)
                ok = ~(cos_x < EPS)
                with np.errstate(all="ignore"):
                    c = Lrad * F * (cos_x * pdf_env / (pdf_env + P) * dom)[:, None]
                ok &= np.isfinite(c).all(-1)
                ok[ok] = tw.visible(qi, one(side[p_], int(ok.sum())), one(pos[p], int(ok.sum())), Ldir[ok], T_MAX)
                out[p] += c[ok].sum(0)
            for lq in sorted({lq for lq, _ in tw.lights}) if tw.nee else []:
                E = tw.quads[lq]
                cc = (np.arange(g_light) + 0.5) / g_light
                A, B = (a.ravel() for a in np.meshgrid(cc, cc))
                sp = E.P0 + A[:, None] * E.E1 + B[:, None] * E.E2
                G = len(sp)
                Lv = sp - pos[p]
                dist2 = _dot(Lv, Lv)
                dist = np.sqrt(dist2)
                Ln = Lv / dist[:, None]
                cos_x, cos_y = Ln @ n[p_], np.abs(Ln @ E.N)
                ok = ~((cos_x < EPS) | (cos_y < EPS))
                F, P = mixture_v(Q.m, one(n[p_], G), Ln, one(wo[p_], G), kdpi[p_], tw.lambert)
                with np.errstate(all="ignore"):
                    pdf_light = tw.light_pdf_area(lq) * dist2 / cos_y
                    mi = pdf_light / (tw.nee * pdf_light + P)
                    c = E.Ke * F * (cos_x * cos_y / dist2 * mi * (E.area / G))[:, None] * tw.nee
                ok &= np.isfinite(c).all(-1)
                ok[ok] = tw.visible(qi, one(side[p_], int(ok.sum())), one(pos[p], int(ok.sum())), Ln[ok], dist[ok], target=lq)
                out[p] += c[ok].sum(0)
    return out


def direct_integral(tw, o, d, g_env=128):
    """the textbook direct lighting of the primary hit by the environment: integral of F L cos+ V d_omega (no MIS weight, no sampler) -> (k, 3); zero where the primary
    ray misses or hits an emitter"""
    k = len(o)
    out = np.zeros((k, 3))
    hq, pos, ha, hb = _primary_points(tw, o, d)
    c = (np.arange(g_env) + 0.5) / g_env
    U, V = (a.ravel() for a in np.meshgrid(c, c))
    Ldir, r3 = tw.env.decode(U, V)
    Lrad, _ = tw.env.eval(Ldir)
    dom = 4.0 / r3 / (g_env * g_env)
    lit = np.nonzero(Lrad.sum(-1) > 0.0)[0]
    Ldir, Lrad, dom = Ldir[lit], Lrad[lit], dom[lit]
    for qi, Q in enumerate(tw.quads):
        sel = np.nonzero(hq == qi)[0]
        if not len(sel) or Q.emits:
            continue
        wo = -d[sel]
        kdpi, plain, n = tw.surface(Q, ha[sel], hb[sel], wo)
        side = np.where(n @ Q.N < 0.0, -1.0, 1.0)
        G = len(Ldir)
        for p_, p in enumerate(sel):
            one = lambda a, cnt: np.broadcast_to(a, (cnt,) + np.shape(a))
            cos_x = Ldir @ n[p_]
            ok = cos_x > 0.0
            F, _ = mixture_v(Q.m, one(n[p_], G), Ldir, one(wo[p_], G), kdpi[p_], tw.lambert)
            cst = Lrad * F * (cos_x * dom)[:, None]
            ok &= np.isfinite(cst).all(-1)
            ok[ok] = tw.visible(qi, one(side[p_], int(ok.sum())), one(pos[p], int(ok.sum())), Ldir[ok], T_MAX)
            out[p] = cst[ok].sum(0)
    return out


# ------------------------------------------------------------------------------------------------
# block statistics
# ------------------------------------------------------------------------------------------------
def block_pixels(width, bx, by, edge=4):
    """row-major pixel ids of block (bx, by)"""
    ys, xs = np.meshgrid(np.arange(by * edge, by * edge + edge), np.arange(bx * edge, bx * edge + edge), indexing="ij")
    return (ys * width + xs).ravel()


def block_samples(tw, rays, pix, n, max_bounces, rng, chunk=1 << 16):
    """n samples of every pixel in pix -> (max_bounces, n, 3): per sample index the MEAN over the block's pixels (pixels are independent, so this is one draw of the
    block statistic whose mean the GPU's block mean estimates)"""
    o, d = rays[pix, 0:3].astype(np.float64), rays[pix, 4:7].astype(np.float64)
    npx = len(pix)
    per = max(1, chunk // npx)
    out = np.zeros((max_bounces, n, 3))
    for s0 in range(0, n, per):
        c = min(per, n - s0)
        r = tw.radiance(np.tile(o, (c, 1)), np.tile(d, (c, 1)), max_bounces, rng)
        out[:, s0:s0 + c] = r.reshape(max_bounces, c, npx, 3).mean(2)
    return out


def moments(x):
    """x (n, ...) samples -> mean, per-sample std, the std of each half, fourth central moment"""
    n = len(x)
    mean = x.mean(0)
    dx = x - mean
    return mean, x.std(0, ddof=1), x[:n // 2].std(0, ddof=1), x[n // 2:].std(0, ddof=1), (dx ** 4).mean(0)

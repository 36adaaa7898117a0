"""The float32 twin of rtx_denoise's two opt-in guide extensions (include/rtx.h, DENOISING: MAP GUIDES), the two scene variants of its tests and their shared inputs.

    map guides   per pixel that is filterable by geometry: A = max(Kd', 2^-6) per channel, Kd' by tests/texture_ref.py at the guide ray's hit record; nm = the normal-mapped
                 shading normal by tests/normalmap_ref.py with wo = the guide ray's direction negated.  Every other pixel: A = (1, 1, 1), nm = (0, 0, 0)
    flag 1       level 0 reads (u1.xyz / max(u1.w, 1)) / A on FILTERABLE pixels, the last level's output of such a pixel is multiplied by A; every other pixel passes through.
                 emulate_maps feeds test_denoise_ref.emulate the pre-divided colours with w in {0, 1} (its own division is then by 1: exact) and multiplies afterwards
    flag 2       dn of the normal stop is taken between nm_p and nm_q; the plane stop keeps n_p.  A copy of emulate's tap loop with that one change
Used by tests/test_denoise_maps_ref.py (no GPU) and tests/test_denoise_maps.py (the device is held to it bit for bit)."""
import functools

import numpy as np

import __graft_entry__ as graft
import normalmap_ref as nr
import test_denoise_ref as ref
import texture_ref as tr
from test_denoise_ref import F, HW, MISS, NOGEO, shifted
from test_normalmap import H, M_A, M_B, M_NONE, NrmScene, W, World

ALBEDO, MAPPED_NORMALS = 1, 2
FLOOR = F(0.015625)
SIZES = ((W, H), (37, 19), (8, 8))
SIGMA_COLOR, SIGMA_PLANE, NORMAL_POWER_LOG2 = 0.5, 0.0625, 5      # sigma_plane: 2^-6 of the room's extent of 4
KW = dict(sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE, normal_power_log2=NORMAL_POWER_LOG2)
LUMA = np.array([0.75, 0.5, 0.25], F)                               # the irradiance of the synthetic accumulation: u1 = A * LUMA, w = 1
REL = 2.0 ** -18
FLOOR_TEX = 4                                                       # the texture id of the 4 x 4 texture of bytes 0, 2 and 255


@functools.lru_cache(maxsize=None)
def world():
    return World(graft.load_package())


@functools.lru_cache(maxsize=None)
def variant(name):
    """KD: map_Kd on M_A (texture 0, linear), M_B (texture 1, sRGB, 3 x 5) and M_NONE (a 4 x 4 texture of bytes 0, 2 and 255: with Kd = 0.5 the first two lie under the floor),
    the normal maps of world.mapped, no opacity maps.  KD+CUT: world.mapped itself (M_ALL carries map_Kd, a cut-out and a normal map)"""
    w = world()
    if name == "KD+CUT":
        return w.mapped
    assert name == "KD"
    px = np.random.default_rng(11).choice(np.array([0, 2, 255], np.uint8), (4, 4, 4))
    assert all((px[..., :3] == b).any() for b in (0, 2, 255))
    kd_maps = list(w.none)
    kd_maps[M_A], kd_maps[M_B], kd_maps[M_NONE] = 0, 1, FLOOR_TEX
    return NrmScene(w.plain, w.uvs, list(w.textures) + [(px, False)], w.nmaps, kd_maps, None)


class Tables:
    """what the twin reads of a scene: per material the table's Kd, the two map slots and the shading kernel's emitter test; per texture (pixels, srgb); per GLOBAL triangle id
    the corner UVs, the tangent record and the instance; per instance its matrix"""
    def __init__(self, scene):
        rt, w = graft.load_package(), world()
        self.materials = np.asarray(scene.materials, F).reshape(-1, 32)
        self.textures = list(scene.textures)
        self.kd_maps = np.array([-1 if t is None else t for t in (scene.material_maps or w.none)], np.int64)
        self.normal_maps = list(scene.normal_maps)
        self.emits = nr.emits_device(self.materials, rt.half_round)
        self.tri_uv, self.tri_tan, self.o2w = w.tables(scene.meshes, scene.instances)
        self.tri_inst = np.concatenate([np.full(len(scene.meshes[mesh][1]) // 3, k, np.uint32) for k, (mesh, _) in enumerate(scene.instances)])
        self.half_round = rt.half_round


def map_guides(tab, rays8, hits4, guides):
    """(H, W, 8) float32 as rtx_debug_denoise_map_guides lays them out: A3, 0, nm3, 0.  rays8 / hits4: the guide rays (primary rays, flags 0) and their closest hits;
    guides: the (H, W, 8) guide record of the same pixels (its material word says which pixels are filterable by geometry, its n is the surface normal)"""
    g = np.ascontiguousarray(guides, F)
    h, w = g.shape[:2]
    g = g.reshape(-1, 8)
    rays = np.asarray(rays8, F).reshape(-1, 8); hits = np.array(hits4, F, copy=True).reshape(-1, 4)
    mat = g[:, 3].view(np.uint32)
    geo = np.nonzero(mat != NOGEO)[0]
    prim = hits[:, 3].view(np.uint32)
    assert (prim[geo] != MISS).all()
    out = np.zeros((h * w, 8), F)
    out[:, 0:3] = F(1)
    # A = max(Kd', 2^-6)
    m = mat[geo].astype(np.int64)
    kd = tr.half_round_array(tab.half_round, tab.materials[m][:, :3])
    tex = tab.kd_maps[m]
    s, t = tr.interp_uv(tab.tri_uv[prim[geo]], hits[geo, 1], hits[geo, 2])
    for k, (px, srgb) in enumerate(tab.textures):
        sel = tex == k
        if sel.any():
            kd[sel] = tr.kd_prime(tab.half_round, tab.materials[m[sel]][:, :3], tr.sample(px, srgb, s[sel], t[sel]))
    A = np.maximum(kd, FLOOR)
    assert A.dtype == F
    out[geo, 0:3] = A
    # nm = n' of the probe, fed the guides' own normal and material and the triangle's instance
    surf = np.zeros((h * w, 16), F)
    surf[:, 4:7] = g[:, 4:7]
    surf[:, 3].view(np.uint32)[:] = mat
    surf[:, 8].view(np.uint32)[geo] = tab.tri_inst[prim[geo]]
    hits[:, 3].view(np.uint32)[mat == NOGEO] = MISS
    nm = nr.shading_normal_probe(tab.textures, tab.normal_maps, tab.emits, tab.tri_uv, tab.tri_tan, surf, tab.o2w, rays, hits)
    out[geo, 4:7] = nm[geo, :3]
    return out.reshape(h, w, 8)


def filter_nm(accum, guides, nm, levels, sigma_color, sigma_plane, normal_power_log2, tally=None):
    """test_denoise_ref.emulate with ONE change: dn = (nm_p.x*nm_q.x + nm_p.y*nm_q.y) + nm_p.z*nm_q.z; the plane stop keeps the guides' n_p.
    tally (optional): per level the taps that count, and those of them whose wn is LOWER than the guides' own normals would give"""
    a = np.ascontiguousarray(accum, F)
    g = np.ascontiguousarray(guides, F)
    nm = np.ascontiguousarray(nm, F)
    h, w = a.shape[:2]
    cnt = np.maximum(a[..., 3], F(1))
    c = a[..., :3] / cnt[..., None]
    P, n, mat = g[..., 0:3], g[..., 4:7], g[..., 3].view(np.uint32)
    filt = (mat != NOGEO) & (a[..., 3] > 0)
    tapmat = np.where(filt, mat, NOGEO)
    inv_plane, inv_color = F(1.0) / F(sigma_plane), F(1.0) / F(sigma_color)
    inside0 = np.ones((h, w), bool)

    def stop(np_, nq_):
        dn = (np_[..., 0] * nq_[..., 0] + np_[..., 1] * nq_[..., 1]) + np_[..., 2] * nq_[..., 2]
        wn = np.maximum(dn, F(0))
        for _ in range(normal_power_log2):
            wn = wn * wn
        return wn
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(levels):
            s = 1 << i
            isc = inv_color * F(s)
            sx = np.zeros((h, w, 3), F); sw = np.zeros((h, w), F)
            t = dict(counted=0, wn_lower=0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    inside = shifted(inside0, s * dx, s * dy, False)
                    mq = shifted(tapmat, s * dx, s * dy, NOGEO)
                    counts = filt & inside & (mq == mat)
                    cq, Pq, nmq = shifted(c, s * dx, s * dy, 0), shifted(P, s * dx, s * dy, 0), shifted(nm, s * dx, s * dy, 0)
                    wn = stop(nm, nmq)
                    d = Pq - P
                    dp = np.abs((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2])
                    wp = np.maximum(F(1) - dp * inv_plane, F(0))
                    dc = (np.abs(cq[..., 0] - c[..., 0]) + np.abs(cq[..., 1] - c[..., 1])) + np.abs(cq[..., 2] - c[..., 2])
                    wc = np.maximum(F(1) - dc * isc, F(0))
                    wt = ((HW[dy + 2] * HW[dx + 2]) * wn) * (wp * wc)
                    for v in (wn, d, dp, wp, dc, wc, wt, isc, cq):
                        assert v.dtype == F
                    nx = sx + wt[..., None] * cq
                    nw = sw + wt
                    assert nx.dtype == F and nw.dtype == F
                    sx = np.where(counts[..., None], nx, sx); sw = np.where(counts, nw, sw)
                    if tally is not None:
                        t["counted"] += int(counts.sum())
                        t["wn_lower"] += int((counts & (wn < stop(n, shifted(n, s * dx, s * dy, 0)))).sum())
            res = sx / np.where(filt, sw, F(1))[..., None]
            assert res.dtype == F
            c = np.where(filt[..., None], res, c)
            if tally is not None:
                tally.append(t)
    out = np.empty((h, w, 4), F)
    out[..., :3], out[..., 3] = c, F(1)
    return out, int(filt.sum())


def emulate_maps(accum, guides, mguides, levels, flags, sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE, normal_power_log2=NORMAL_POWER_LOG2, tally=None):
    """-> (denoised (H, W, 4) float32, pixels filtered) of rtx_denoise with `flags` (0 .. 3)"""
    a = np.ascontiguousarray(accum, F)
    g = np.ascontiguousarray(guides, F)
    mg = np.ascontiguousarray(mguides, F)
    A, nm = mg[..., 0:3], mg[..., 4:7]
    filt = (g[..., 3].view(np.uint32) != NOGEO) & (a[..., 3] > 0)
    if flags & ALBEDO:
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            mean = a[..., :3] / np.maximum(a[..., 3], F(1))[..., None]
            demod = mean / A
        assert mean.dtype == F and demod.dtype == F
        a = np.empty_like(a)
        a[..., :3] = np.where(filt[..., None], demod, mean)
        a[..., 3] = np.where(np.ascontiguousarray(accum, F)[..., 3] > 0, F(1), F(0))
    if flags & MAPPED_NORMALS:
        out, nf = filter_nm(a, g, nm, levels, sigma_color, sigma_plane, normal_power_log2, tally)
    else:
        out, nf = ref.emulate(a, g, levels, sigma_color, sigma_plane, normal_power_log2)
    if flags & ALBEDO:
        with np.errstate(over="ignore", invalid="ignore"):
            mod = out[..., :3] * A
        assert mod.dtype == F
        out[..., :3] = np.where(filt[..., None], mod, out[..., :3])
    assert nf == int(filt.sum())
    return out, nf


def synthetic_accum(mguides):
    """u1.k = A.k * LUMA.k (a float32 product), w = 1: an image whose only detail is the albedo's"""
    a = np.empty(mguides.shape[:2] + (4,), F)
    a[..., :3] = np.ascontiguousarray(mguides, F)[..., 0:3] * LUMA
    a[..., 3] = F(1)
    return a


def rel_err(img, want):
    """max over channels of |img - want| / |want| per pixel, in double"""
    i, w = np.asarray(img, np.float64)[..., :3], np.asarray(want, np.float64)[..., :3]
    return (np.abs(i - w) / np.abs(w)).max(-1)


@functools.lru_cache(maxsize=None)
def oracle_inputs(name, width=W, height=H):
    """the oracle's guide rays, first hits, guide record and the twin's map guides of a variant WITHOUT cut-outs (the oracle knows none); read-only, computed once"""
    assert name == "KD"
    rt, orc = graft.load_package(), graft.load_oracle()
    sc = variant(name)
    o = orc.Oracle().load(sc, W / H)
    rays = o.primary_rays(rt.Params(width=width, height=height, flags=0))
    hits = o.trace_closest(rays, 1)
    o.close()
    g = ref.guides_of(sc, width, height, W / H)
    mg = map_guides(Tables(sc), rays, hits, g)
    for v in (rays, hits, mg):
        v.setflags(write=False)
    return rays, hits, g, mg


def moved_under_flag0(name="KD", levels=5):
    """the synthetic accumulation of a variant through the twin with flags 0: (mask of the filterable pixels of materials with a map_Kd that move by more than 5 %, those pixels)"""
    _, _, g, mg = oracle_inputs(name)
    sc = variant(name)
    mat = g[..., 3].view(np.uint32)
    kd_maps = Tables(sc).kd_maps
    mapped = (mat != NOGEO) & (kd_maps[np.where(mat != NOGEO, mat, 0).astype(np.int64)] >= 0)
    a = synthetic_accum(mg)
    d0, _ = emulate_maps(a, g, mg, levels, 0)
    return mapped & (rel_err(d0, a) > 0.05), mapped

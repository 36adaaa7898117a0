"""numpy emulation of the emission maps as include/rtx.h defines them (EMISSION MAPS): the commit-time quadrature that gives a mapped emitter triangle the mean of its texels,
the light weights, their order, the CDF and the per-triangle q; Ke' at an emissive hit; and the first half of a triangle-light NEE sample given a seed.  float32 throughout,
one numpy operation per written operation, built on tests/texture_ref.py's sampler and tests/env_ref.py's TEA generator; the fused dot / cross / matrix products of the
library (csrc/rtx_math.hpp) are replayed as a float64 product and sum rounded once.  Shared by tests/test_emimap_ref.py (its own properties and the host builder, no GPU) and
tests/test_emimap.py (the device is held to it bit for bit)."""
import math

import numpy as np

import env_ref as er
import texture_ref as tr

F = np.float32
MISS = np.uint32(0xFFFFFFFF)
EPS = F(0.000001)
MAX_SPLIT = 16


def fma(a, b, c):
    """a * b + c rounded once (the product of two float32 is exact in float64)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def dot(a, b):
    return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def cross(a, b):
    return np.stack([fma(a[..., 1], b[..., 2], -(a[..., 2] * b[..., 1])), fma(a[..., 2], b[..., 0], -(a[..., 0] * b[..., 2])), fma(a[..., 0], b[..., 1], -(a[..., 1] * b[..., 0]))], axis=-1)


def length(a):
    return np.sqrt(dot(a, a))


def xform_point(m, p):
    """csrc/rtx_math.hpp: xform_point with the 16 floats of an objectToWorld"""
    m = np.asarray(m, F).reshape(16); p = np.asarray(p, F)
    return np.stack([fma(m[8 + k], p[..., 2], fma(m[4 + k], p[..., 1], fma(m[k], p[..., 0], m[12 + k]))) for k in range(3)], axis=-1)


# ------------------------------------------------------------------------------------------------
# the commit-time mean
# ------------------------------------------------------------------------------------------------
def split(uv3, W, H):
    """n = clamp(ceil(max over the three edges of max(|du| * W, |dv| * H)), 1, 16), in double"""
    uv = np.asarray(uv3, np.float32).astype(np.float64).reshape(3, 2)
    m = 0.0
    for a, b in ((0, 1), (1, 2), (2, 0)):
        m = max(m, abs(uv[b, 0] - uv[a, 0]) * W, abs(uv[b, 1] - uv[a, 1]) * H)
    return int(min(max(math.ceil(m), 1), MAX_SPLIT))


def centroids(n):
    """hit barycentrics (u, v) of the n^2 sub-triangles' centroids, double: i outer, j inner, the upright one of a cell before its inverted one"""
    out = []
    for i in range(n):
        for j in range(n - i):
            out.append(((i + 1.0 / 3.0) / n, (j + 1.0 / 3.0) / n))
            if i + j <= n - 2:
                out.append(((i + 2.0 / 3.0) / n, (j + 2.0 / 3.0) / n))
    return np.array(out, np.float64)


def triangle_mean(rgba8, srgb, uv3):
    """mean[k] of Sample() over the triangle: the centroids rounded to float32, b0 / s / t / Sample in float32 as at a hit, the sum in double in order, / n^2, rounded once"""
    px = np.asarray(rgba8, np.uint8)
    n = split(uv3, px.shape[1], px.shape[0])
    c = centroids(n).astype(np.float32)
    assert len(c) == n * n
    s, t = tr.interp_uv(np.repeat(np.asarray(uv3, np.float32).reshape(1, 3, 2), len(c), axis=0), c[:, 0], c[:, 1])
    tl = tr.sample(px, srgb, s, t).astype(np.float64)
    total = np.zeros(3, np.float64)
    for row in tl:                                                            # (in order: a double sum is not associative either)
        total = total + row
    return (total / float(n * n)).astype(np.float32)


def triangle_weight_terms(half_round, ke_full, mean):
    """E = KeFull * mean (float32), inten = (E.x + E.y + E.z) / 3, q = (Eh.x + Eh.y + Eh.z) / 3 with Eh = half_round(E)"""
    E = np.asarray(ke_full, np.float32) * np.asarray(mean, np.float32)
    inten = ((E[0] + E[1]) + E[2]) / F(3.0)
    Eh = tr.half_round_array(half_round, E)
    q = ((Eh[0] + Eh[1]) + Eh[2]) / F(3.0)
    return E, inten, q


# ------------------------------------------------------------------------------------------------
# the light list of a scene
# ------------------------------------------------------------------------------------------------
class LightList:
    """what rtx_commit_scene derives for the lights of a scene given as arrays (materials (n, 32); meshes [(verts (n, 7), indices, material ids per index entry)]; uvs per
    mesh (index count, 2) or None; instances [(mesh, objectToWorld 16)]; textures [(pixels (H, W, 4) uint8, srgb)]; ke_maps per material a texture id or -1 / None):
    records (n, 20) float32 as rtx_get_lights hands them out, prim / tex per light, q per global triangle id, total, and the device's world-space half"""
    def __init__(self, half_round, materials, meshes, uvs, instances, textures, ke_maps, hidden=()):
        mats = np.asarray(materials, np.float32)
        ke_maps = list(ke_maps) if ke_maps is not None else []
        tex_of = lambda m: (ke_maps[m] if m < len(ke_maps) and ke_maps[m] is not None else -1)
        emits = lambda m: bool((mats[m, 8:11] > 0).any())
        tri_base, nt = [], 0
        for mesh, _ in instances:
            tri_base.append(nt); nt += len(meshes[mesh][1]) // 3
        self.active = any(emits(int(m)) and tex_of(int(m)) >= 0 for mesh, _ in instances for m in np.asarray(meshes[mesh][2])[::3])
        self.q = np.zeros(nt, np.float32)
        tmp = []
        for ii, (mesh, o2w) in enumerate(instances):
            if ii in hidden:
                continue
            v, idx, mid = meshes[mesh]
            v = np.asarray(v, np.float32).reshape(-1, 7); idx = np.asarray(idx, np.int64); mid = np.asarray(mid, np.int64)
            for t in range(len(idx) // 3):
                m0, m1, m2 = (int(x) for x in mid[3 * t:3 * t + 3])
                if m0 >= len(mats):
                    continue
                ke = mats[m0, 8:11]
                ksum = (ke[0] + ke[1]) + ke[2]
                inten = ksum / F(3.0)
                tex = -1
                if self.active and ksum > 0:
                    tex = tex_of(m0) if emits(m0) else -1
                    mean = np.ones(3, np.float32)
                    if tex >= 0:
                        uv3 = np.asarray(uvs[mesh], np.float32).reshape(-1, 3, 2)[t] if uvs[mesh] is not None else np.zeros((3, 2), np.float32)
                        mean = triangle_mean(textures[tex][0], textures[tex][1], uv3)
                        _, inten, q = triangle_weight_terms(half_round, ke, mean)
                    else:
                        kh = tr.half_round_array(half_round, ke)
                        q = ((kh[0] + kh[1]) + kh[2]) / F(3.0)
                    self.q[tri_base[ii] + t] = q
                if m0 != m1 or m0 != m2 or not ksum > 0:
                    continue
                p = v[idx[3 * t:3 * t + 3], :3]
                area = F(0.5) * length(cross(p[1] - p[0], p[2] - p[0]))
                tmp.append(dict(w=F(area * inten), order=len(tmp), inst=ii, p=p, em=ke.copy(), prim=tri_base[ii] + t, tex=tex))
        tmp.sort(key=lambda L: (-float(L["w"]), L["order"]))
        total = F(0.0)
        for L in tmp:
            total = F(total + L["w"])
        self.total = total
        n = len(tmp)
        self.records = np.zeros((n, 20), np.float32)
        self.prim = np.array([L["prim"] for L in tmp], np.uint32)
        self.tex = np.array([L["tex"] for L in tmp], np.int32)
        self.points = np.zeros((n, 3, 3), np.float32); self.pdf_l = np.zeros(n, np.float32)
        cum = F(0.0)
        for i, L in enumerate(tmp):
            with np.errstate(divide="ignore", invalid="ignore"):
                wn = F(0.0) if (self.active and not total > 0) else F(L["w"] / total)
            cum = F(cum + wn)
            r = self.records[i]
            r[0:3] = L["p"][0]; r[3] = F(1.0) if i + 1 == n else cum
            r[4:7] = L["p"][1]; r[7:8].view(np.uint32)[0] = L["inst"]
            r[8:11] = L["p"][2]; r[11] = wn
            r[12:15] = L["em"]; r[15:16].view(np.uint32)[0] = n
            r[16] = total
            w = xform_point(instances[L["inst"]][1], L["p"])
            self.points[i] = w
            area_l = np.abs(length(cross(w[1] - w[0], w[2] - w[0])) * F(0.5))
            self.pdf_l[i] = max(EPS, F(wn / max(area_l, EPS)))
        self.cdf = self.records[:, 3].copy()
        self.nlights = 0 if (self.active and not total > 0) else n      # what the renderer samples: nothing when every map is black


# ------------------------------------------------------------------------------------------------
# the two probes
# ------------------------------------------------------------------------------------------------
def emits_device(half_round, materials):
    """per material: the rounded Ke has length > 0 (MatGPU::Ke_len; any non-zero component)"""
    ke = tr.half_round_array(half_round, np.asarray(materials, np.float32)[:, 8:11])
    return (ke != 0).any(axis=1)


def emission_probe(half_round, textures, ke_maps, materials, q, tri_mat, tri_uv, hits4, active=True):
    """rtx_debug_emission -> ((n, 4) float32: Ke', q[prim]; (n,) uint32 texture ids): Ke'[k] = half_round(KeFull[k] * tl[k]) on a mapped emitter, the table's Ke on an
    unmapped one, zeros and 0xFFFFFFFF for a non-emitter or a miss.  active=False: no emission map is active — the table's Ke, its mean, no texture"""
    mats = np.asarray(materials, np.float32)
    hits = np.asarray(hits4, np.float32).reshape(-1, 4)
    prim = hits[:, 3].copy().view(np.uint32)
    hit = prim != MISS
    p = np.where(hit, prim, 0)
    mat = np.asarray(tri_mat)[p]
    em = emits_device(half_round, mats)
    ke_tab = tr.half_round_array(half_round, mats[:, 8:11])
    out = np.zeros((len(hits), 4), np.float32); ids = np.full(len(hits), MISS, np.uint32)
    sel = hit & em[mat]
    out[sel, :3] = ke_tab[mat[sel]]
    if not active:
        out[sel, 3] = ((out[sel, 0] + out[sel, 1]) + out[sel, 2]) / F(3.0)
        return out, ids
    out[sel, 3] = np.asarray(q, np.float32)[p[sel]]
    s, t = tr.interp_uv(np.asarray(tri_uv, np.float32)[p], hits[:, 1], hits[:, 2])
    for m in range(len(mats)):
        tex = ke_maps[m] if ke_maps is not None and m < len(ke_maps) and ke_maps[m] is not None else -1
        k = sel & (mat == m)
        if tex < 0 or not k.any():
            continue
        tl = tr.sample(textures[tex][0], textures[tex][1], s[k], t[k])
        out[k, :3] = tr.half_round_array(half_round, mats[m, 8:11] * tl)
        ids[k] = tex
    return out, ids


def light_sample(L, textures, tri_uv, seeds, active=True):
    """rtx_debug_light_sample on the light list L (LightList) at (n, 2) uint32 seeds -> dict like Context.light_sample's: the selection draw and the CDF search, the two
    area draws and their fold, the sampled point (fused, as lincomb3), s / t and em * tl for a light with the map (else 0, 0 and em), pdf_l, the seed after"""
    seeds = np.asarray(seeds, np.uint32).reshape(-1, 2)
    rv, s0, s1 = er.tea_next(seeds[:, 0], seeds[:, 1])
    sel = er.search(L.cdf[None, :L.nlights], rv)
    xi1, s0, s1 = er.tea_next(s0, s1)
    xi2, s0, s1 = er.tea_next(s0, s1)
    fold = xi1 + xi2 > F(1.0)
    xi1, xi2 = np.where(fold, F(1.0) - xi1, xi1), np.where(fold, F(1.0) - xi2, xi2)
    u, v, w = F(1.0) - xi1 - xi2, xi1, xi2
    P = L.points[sel]
    point = np.stack([fma(P[:, 2, k], w, fma(P[:, 1, k], v, P[:, 0, k] * u)) for k in range(3)], axis=-1)
    st = np.zeros((len(seeds), 2), np.float32)
    em = L.records[sel, 12:15].copy()
    if active:
        uv3 = np.asarray(tri_uv, np.float32)[L.prim[sel]]
        s = (u * uv3[:, 0, 0] + v * uv3[:, 1, 0]) + w * uv3[:, 2, 0]
        t = (u * uv3[:, 0, 1] + v * uv3[:, 1, 1]) + w * uv3[:, 2, 1]
        for tex in set(int(x) for x in L.tex[sel] if x >= 0):
            k = L.tex[sel] == tex
            st[k, 0], st[k, 1] = s[k], t[k]
            em[k] = em[k] * tr.sample(textures[tex][0], textures[tex][1], s[k], t[k])
    return dict(light=sel.astype(np.uint32), point=point, st=st, em=em, pdf_l=L.pdf_l[sel], seed=np.stack([s0, s1], axis=-1))

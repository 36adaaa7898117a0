"""numpy emulation of the tangent-space normal maps as include/rtx.h defines them (NORMAL MAPS): the decode table Nt, the per-triangle tangent records (double, rounded
once), the shading normal n' of a hit, and the two image helpers of the host layer (height map -> normal map, green flip), on the addressing of tests/texture_ref.py.
float32 on the device side and float64 on the host side, one numpy operation per written operation (numpy never contracts a multiply and an add).  Shared by
tests/test_normalmap_ref.py (its own properties, no GPU) and tests/test_normalmap.py (the device is held to it bit for bit)."""
import numpy as np

import texture_ref as tr

F = np.float32
NO_TEX = np.uint32(0xFFFFFFFF)


def table():
    """Nt[b] = max(((float)b - 128.0f) / 127.0f, -1.0f)"""
    return np.maximum((np.arange(256, dtype=np.float32) - F(128.0)) / F(127.0), F(-1.0))


def tangent_records(p3, uv3):
    """p3 (n, 3, 3) float32 object-space corners, uv3 (n, 3, 2) float32 corner pairs -> (n, 6) float32: T, B; zeros where det == 0 or a value is not finite as float32"""
    p = np.asarray(p3, np.float32).astype(np.float64).reshape(-1, 3, 3)
    uv = np.asarray(uv3, np.float32).astype(np.float64).reshape(-1, 3, 2)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    du1, dv1 = uv[:, 1, 0] - uv[:, 0, 0], uv[:, 1, 1] - uv[:, 0, 1]
    du2, dv2 = uv[:, 2, 0] - uv[:, 0, 0], uv[:, 2, 1] - uv[:, 0, 1]
    det = du1 * dv2 - du2 * dv1
    with np.errstate(all="ignore"):
        T = (e1 * dv2[:, None] - e2 * dv1[:, None]) / det[:, None]
        B = (e2 * du1[:, None] - e1 * du2[:, None]) / det[:, None]
        out = np.concatenate([T, B], axis=1).astype(np.float32)
    bad = (det == 0.0) | ~np.isfinite(out).all(axis=1)
    out[bad] = F(0.0)
    return out


def decode(rgba8, s, t):
    """c = the bilinear sample of the RGB bytes through Nt -> (n, 3) float32"""
    px = np.asarray(rgba8, np.uint8)
    T = table()
    ix0, ix1, iy0, iy1, fx, fy = tr.taps(px.shape, s, t)
    out = np.zeros((len(fx), 3), np.float32)
    for k in range(3):
        c00, c10, c01, c11 = T[px[iy0, ix0, k]], T[px[iy0, ix1, k]], T[px[iy1, ix0, k]], T[px[iy1, ix1, k]]
        top = c00 + fx * (c10 - c00)
        bot = c01 + fx * (c11 - c01)
        out[:, k] = top + fy * (bot - top)
    assert out.dtype == np.float32
    return out


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def perturb(n, c, tan6, o2w, wo, branches=None):
    """n' for n (k, 3) world shading normals, c (k, 3) decoded texels, tan6 (k, 6) tangent records, o2w (k, 16) instance matrices (M[4 * column + row]), wo (k, 3).
    float32 in the written order.  branches (a dict, optional) receives boolean masks: flat, degenerate (no tangent), zero (m2 not usable), guard"""
    n, c, tan6, M, wo = (np.ascontiguousarray(a, np.float32) for a in (n, c, tan6, o2w, wo))
    k = len(n)
    out = n.copy()
    with np.errstate(all="ignore"):
        flat = (c[:, 0] == 0) & (c[:, 1] == 0)
        Tw = np.stack([(M[:, 0 + j] * tan6[:, 0] + M[:, 4 + j] * tan6[:, 1]) + M[:, 8 + j] * tan6[:, 2] for j in range(3)], axis=1)
        Bw = np.stack([(M[:, 0 + j] * tan6[:, 3] + M[:, 4 + j] * tan6[:, 4]) + M[:, 8 + j] * tan6[:, 5] for j in range(3)], axis=1)
        dT = _dot(n, Tw)
        tv = Tw - n * dT[:, None]
        l2 = _dot(tv, tv)
        degenerate = ~flat & (~(l2 > 0) | np.isinf(l2))
        inv = F(1.0) / np.sqrt(l2)
        t = tv * inv[:, None]
        bv = np.stack([n[:, 1] * t[:, 2] - n[:, 2] * t[:, 1], n[:, 2] * t[:, 0] - n[:, 0] * t[:, 2], n[:, 0] * t[:, 1] - n[:, 1] * t[:, 0]], axis=1)
        sg = np.where(_dot(bv, Bw) < 0, F(-1.0), F(1.0)).astype(np.float32)
        m = (t * c[:, 0:1] + (bv * sg[:, None]) * c[:, 1:2]) + n * c[:, 2:3]
        m2 = _dot(m, m)
        live = ~flat & ~degenerate
        zero = live & (~(m2 > 0) | np.isinf(m2))
        npr = m * (F(1.0) / np.sqrt(m2))[:, None]
        a, ap = _dot(n, wo), _dot(npr, wo)
        live = live & ~zero
        guard = live & (((a > 0) & ~(ap > 0)) | ((a < 0) & ~(ap < 0)))
    use = live & ~guard
    out[use] = npr[use]
    assert out.dtype == np.float32 and npr.dtype == np.float32 and len(out) == k
    if branches is not None:
        branches.update(flat=flat, degenerate=degenerate, zero=zero, guard=guard)
    return out


def emits_device(materials, half_round):
    """per material: the shading kernel's emitter test, length(half_round(Ke)) > 0, i.e. some component of Ke survives the half-precision rounding of the material table"""
    ke = np.asarray(materials, np.float32).reshape(-1, 32)[:, 8:11]
    return np.array([any(half_round(float(x)) != 0.0 for x in row) for row in ke], bool)


def shading_normal_probe(textures, normal_maps, emits, tri_uv3, tri_tan, surf, o2w_of_inst, rays, hits, branches=None):
    """(n, 4) float32 as Context.shading_normal returns it.  textures: list of (H, W, 4) uint8 (or (array, srgb) pairs); normal_maps: per material a texture id or -1;
    emits: per material bool; tri_uv3 (ntri, 3, 2); tri_tan (ntri, 6); surf = Context.surface(rays, hits) (n, 16): its normal, material and instance are the inputs;
    o2w_of_inst (ninst, 16)"""
    rays = np.asarray(rays, np.float32).reshape(-1, 8); hits = np.asarray(hits, np.float32).reshape(-1, 4); surf = np.asarray(surf, np.float32).reshape(-1, 16)
    prim = hits[:, 3].view(np.uint32)
    out = np.zeros((len(hits), 4), np.float32)
    out[:, 3].view(np.uint32)[:] = NO_TEX
    hit = prim != NO_TEX
    out[hit, :3] = surf[hit, 4:7]
    mat = surf[:, 3].view(np.uint32).astype(np.int64); inst = surf[:, 8].view(np.uint32).astype(np.int64)
    nm = np.array([-1 if t is None else t for t in normal_maps], np.int64)
    ok = hit & (mat < len(nm))
    tex = np.full(len(hits), -1, np.int64)
    tex[ok] = np.where(np.asarray(emits, bool)[mat[ok]], -1, nm[mat[ok]])
    masks = {k: np.zeros(len(hits), bool) for k in ("flat", "degenerate", "zero", "guard")}
    for k, t in enumerate(textures):
        px = t[0] if isinstance(t, tuple) else t
        sel = np.nonzero(tex == k)[0]
        if not len(sel):
            continue
        s, tt = tr.interp_uv(np.asarray(tri_uv3, np.float32)[prim[sel]], hits[sel, 1], hits[sel, 2])
        c = decode(px, s, tt)
        br = {}
        out[sel, :3] = perturb(surf[sel, 4:7], c, np.asarray(tri_tan, np.float32)[prim[sel]], np.asarray(o2w_of_inst, np.float32).reshape(-1, 16)[inst[sel]], -rays[sel, 4:7], br)
        out[:, 3].view(np.uint32)[sel] = np.uint32(k)
        for name in masks:
            masks[name][sel] = br[name]
    if branches is not None:
        branches.update(masks)
    return out


def height_to_normal(rgba8, strength):
    """HeightToNormalMap: channel 0 as a height map (h = byte / 255, repeat wrap, row 0 on top so v runs upward) -> (H, W, 4) uint8 normal map; float64"""
    px = np.asarray(rgba8, np.uint8)
    h = px[..., 0].astype(np.float64) / 255.0
    S = float(strength)
    gx = (np.roll(h, -1, axis=1) - np.roll(h, 1, axis=1)) * 0.5 * S            # h[x + 1] - h[x - 1]
    gy = (np.roll(h, 1, axis=0) - np.roll(h, -1, axis=0)) * 0.5 * S            # h[row - 1] - h[row + 1]
    ln = np.sqrt((gx * gx + gy * gy) + 1.0)
    c = np.stack([-gx / ln, -gy / ln, 1.0 / ln], axis=-1)
    out = np.full(px.shape[:2] + (4,), 255, np.uint8)
    out[..., :3] = np.clip(np.floor(c * 127.0 + 128.5), 0.0, 255.0).astype(np.uint8)
    return out


def flip_green(rgba8):
    """FlipGreen: g' = g == 0 ? 255 : 256 - g (an exact negation under Nt)"""
    out = np.array(rgba8, np.uint8, copy=True)
    g = out[..., 1].astype(np.int32)
    out[..., 1] = np.where(g == 0, 255, 256 - g).astype(np.uint8)
    return out

"""numpy emulation of the alpha cut-outs as include/rtx.h defines them (ALPHA CUT-OUTS): the alpha of an opacity texture at a hit and the acceptance test, on the addressing
of tests/texture_ref.py.  float32 throughout, one numpy operation per written operation.  Shared by tests/test_cutout_ref.py (its own properties, no GPU) and
tests/test_cutout.py (the device is held to it bit for bit)."""
import numpy as np

import texture_ref as tr

F = np.float32
CUT_OFF = F(0.5)
NO_TEX = np.uint32(0xFFFFFFFF)


def alpha(rgba8, s, t):
    """the alpha of Sample's four taps through the LINEAR table (whatever the texture's encoding), the same two lerps as a colour channel -> (n,) float32"""
    px = np.asarray(rgba8, np.uint8)
    T = tr.table(False)
    ix0, ix1, iy0, iy1, fx, fy = tr.taps(px.shape, s, t)
    a00, a10, a01, a11 = T[px[iy0, ix0, 3]], T[px[iy0, ix1, 3]], T[px[iy1, ix0, 3]], T[px[iy1, ix1, 3]]
    top = a00 + fx * (a10 - a00)
    bot = a01 + fx * (a11 - a01)
    out = top + fy * (bot - top)
    assert out.dtype == np.float32
    return out


def accepted(a):
    """the hit counts iff a >= 0.5f"""
    return np.asarray(a, np.float32) >= CUT_OFF


def alpha_at(rgba8, uv3, u, v):
    """alpha at barycentrics (u, v) of triangles whose corner pairs are uv3 (n, 3, 2)"""
    s, t = tr.interp_uv(uv3, u, v)
    return alpha(rgba8, s, t)


def alpha_taps_agree(rgba8, s, t):
    """per sample: the four taps read the same alpha byte (the alpha is then T[byte] exactly)"""
    px = np.asarray(rgba8, np.uint8)[..., 3]
    ix0, ix1, iy0, iy1, _, _ = tr.taps(px.shape, s, t)
    a = px[iy0, ix0]
    return (px[iy0, ix1] == a) & (px[iy1, ix0] == a) & (px[iy1, ix1] == a)


def emits(materials):
    """per material: a component of Ke is > 0"""
    return (np.asarray(materials, np.float32)[:, 8:11] > 0).any(axis=1)


def cut_textures(materials, opacity_maps, tri_mat):
    """per triangle (its material = the id of its first index entry): the opacity texture of a cut-out triangle, or -1"""
    om = np.array([-1 if t is None else t for t in opacity_maps] + [-1] * (len(materials) - len(opacity_maps)), np.int64)
    om = np.where(emits(materials), -1, om)
    return om[np.asarray(tri_mat, np.int64)]


def opacity_probe(textures, tri_cut, tri_uv3, hits):
    """(n, 2) float32 as Context.opacity returns it: (alpha, texture id bits); (1, 0xFFFFFFFF) for a miss and for a triangle that is not a cut-out triangle"""
    hits = np.asarray(hits, np.float32).reshape(-1, 4)
    prim = hits[:, 3].view(np.uint32)
    out = np.ones((len(hits), 2), np.float32)
    out[:, 1].view(np.uint32)[:] = NO_TEX
    hit = np.nonzero(prim != NO_TEX)[0]
    tex = np.asarray(tri_cut, np.int64)[prim[hit]]
    for k, t in enumerate(textures):
        px = t[0] if isinstance(t, tuple) else t
        sel = hit[tex == k]
        if len(sel):
            out[sel, 0] = alpha_at(px, tri_uv3[prim[sel]], hits[sel, 1], hits[sel, 2])
            out[:, 1].view(np.uint32)[sel] = np.uint32(k)
    return out

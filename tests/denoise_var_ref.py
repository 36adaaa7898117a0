"""The float32 twin of rtx_denoise_variance (include/rtx.h, DENOISING: VARIANCE-GUIDED), built on the taps of tests/test_denoise_ref.py and the map guides of
tests/denoise_maps_ref.py.

    level-0 input   a = u1, hb = `half` (the running sum of the odd sample ids, tests/test_adaptive_ref.py); for a pixel with a.w > 0
                        cnt = max(a.w, 1);  c = a.xyz / cnt;  e = (a.xyz - (hb.xyz + hb.xyz)) / cnt;  under flag 1, filterable pixels only: c = c / A, e = e / A
                        el = (0.2126 e.x + 0.7152 e.y) + 0.0722 e.z;  v = el * el
    every level     gv = the 3 x 3 binomial mean of v over the positions ONE pixel apart that count (inside, filterable, the centre's material), sequential from 0;
                    inv = 1 / (sigma_var * sqrt(gv) + 2^-20);  wc = max(1 - |l_q - l_p| * inv, 0) with l the luminance of this level's input colour;
                    w = ((h h) wn) (wp wc);  sum += w c_q;  sumw += w;  sumv += (w w) v_q;  c = sum / sumw,  v = sumv / (sumw sumw)
The taps are visited one after the other for the whole image at once (a shifted view per tap), which is the sequential per-pixel order of the kernel.
Used by tests/test_denoise_var_ref.py (no GPU) and tests/test_denoise_var.py (the device is held to it bit for bit)."""
import functools

import numpy as np

import test_adaptive_ref as ar
import test_denoise_ref as ref
from denoise_maps_ref import ALBEDO, MAPPED_NORMALS
from test_denoise_ref import F, HW, NOGEO, shifted

SIGMA_VAR = 4.0
EPS = F(9.5367431640625e-07)                                        # 2^-20: part of the definition
LR, LG, LB = F(0.2126), F(0.7152), F(0.0722)
GW = np.array([1 / 16, 1 / 8, 1 / 16, 1 / 8, 1 / 4, 1 / 8, 1 / 16, 1 / 8, 1 / 16], F)


class Emulation(ar.Emulation):
    """tests/test_adaptive_ref.py's emulation with `half` as include/rtx.h and k_accumulate define it: the running sum of the ODD sample ids.
    render_adaptive hands _add `1 - (sample_base & 1)` under the name base_is_odd, so with the tests' odd sample_base the parent class sums the EVEN ids into `half`.  The
    criterion reads only |u1 - (half + half)|, which is the same distance from either half up to rounding, so u1, the counts and every decision of the tests' frames are
    the same (tests/test_denoise_var_ref.py asserts it); `half` itself is not.  The filter reads `half`, so its twin needs the sum the device keeps"""
    def _add(self, chunks, frames, first, nsamples, base_is_odd):
        return super()._add(chunks, frames, first, nsamples, 1 - base_is_odd)


@functools.lru_cache(maxsize=None)
def emulate(flags, tile_size, max_spp=ar.MAX_SPP, threshold=ar.THRESHOLD):
    """test_adaptive_ref.emulate on the corrected class -> (Emulation, result dict); shared and read-only"""
    e = Emulation(ar.W, ar.H, tile_size)
    res = e.render_adaptive(ar.oracle_frames(flags), ar.BASE["sample_base"], ar.MIN_SPP, ar.STEP_SPP, max_spp, threshold)
    e.accum.setflags(write=False); e.half.setflags(write=False)
    return e, res


def luminance(c):
    l = (LR * c[..., 0] + LG * c[..., 1]) + LB * c[..., 2]
    assert l.dtype == F
    return l


def filterable(a, guides):
    return (np.ascontiguousarray(guides, F)[..., 3].view(np.uint32) != NOGEO) & (np.ascontiguousarray(a, F)[..., 3] > 0)


def variance_input(a, hb, A=None, filt=None):
    """-> (c (H, W, 3), v (H, W)) float32: the level-0 input.  A (with filt, the filterable mask): RTX_DENOISE_ALBEDO's divisor, applied to filterable pixels only.
    Pixels with a.w == 0 get their mean (u1.xyz / 1) and v = 0; they are read by nothing"""
    a, hb = np.ascontiguousarray(a, F), np.ascontiguousarray(hb, F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        cnt = np.maximum(a[..., 3], F(1))
        c = a[..., :3] / cnt[..., None]
        e = (a[..., :3] - (hb[..., :3] + hb[..., :3])) / cnt[..., None]
        if A is not None:
            A = np.ascontiguousarray(A, F)
            c = np.where(filt[..., None], c / A, c)
            e = np.where(filt[..., None], e / A, e)
        el = luminance(e)
        v = el * el
    assert c.dtype == F and e.dtype == F and v.dtype == F
    return c, np.where(a[..., 3] > 0, v, F(0))


def prefilter(v, filt, mat, tapmat):
    """gv per pixel (meaningful on filterable pixels): sg / sgw over the nine positions one pixel apart that count"""
    h, w = v.shape
    inside0 = np.ones((h, w), bool)
    sg = np.zeros((h, w), F); sgw = np.zeros((h, w), F)
    k = 0
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                counts = filt & shifted(inside0, dx, dy, False) & (shifted(tapmat, dx, dy, NOGEO) == mat)
                ng = sg + GW[k] * shifted(v, dx, dy, 0)
                nw = sgw + GW[k]
                assert ng.dtype == F and nw.dtype == F
                sg = np.where(counts, ng, sg); sgw = np.where(counts, nw, sgw)
                k += 1
        gv = sg / np.where(filt, sgw, F(1))
    assert gv.dtype == F
    return gv


def emulate_var(a, hb, guides, mguides, levels, flags=0, sigma_var=SIGMA_VAR, sigma_plane=ref.SIGMA_PLANE, normal_power_log2=ref.NORMAL_POWER_LOG2, tally=None):
    """-> (denoised (H, W, 4) float32, pixels filtered) of rtx_denoise_variance with `flags` (0 .. 3).  mguides may be None while flags == 0.
    tally (optional): a list that receives per level a dict: taps of filterable centres that count, those the colour stop alone rejects, those with 0 < wc < 1, the filterable
    pixels with gv != v and with v == 0, and the median of v over the filterable pixels (this level's INPUT variance)"""
    a = np.ascontiguousarray(a, F)
    g = np.ascontiguousarray(guides, F)
    h, w = a.shape[:2]
    P, n, mat = g[..., 0:3], g[..., 4:7], g[..., 3].view(np.uint32)
    filt = (mat != NOGEO) & (a[..., 3] > 0)
    tapmat = np.where(filt, mat, NOGEO)
    A = nm = None
    if flags:
        mg = np.ascontiguousarray(mguides, F)
        A, nm = mg[..., 0:3], mg[..., 4:7]
    c, v = variance_input(a, hb, A if flags & ALBEDO else None, filt)
    ns = nm if flags & MAPPED_NORMALS else n                 # the normals of the normal stop; the plane stop keeps n
    inv_plane, sv = F(1.0) / F(sigma_plane), F(sigma_var)
    inside0 = np.ones((h, w), bool)
    assert inv_plane.dtype == F and sv.dtype == F
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for i in range(levels):
            s = 1 << i
            gv = prefilter(v, filt, mat, tapmat)
            inv = F(1.0) / (sv * np.sqrt(gv) + EPS)
            lp = luminance(c)
            assert inv.dtype == F
            sx = np.zeros((h, w, 3), F); sw = np.zeros((h, w), F); svv = np.zeros((h, w), F)
            t = dict(counted=0, wc0=0, partial=0, filterable=int(filt.sum()), gv_ne_v=int((filt & (gv != v)).sum()), v_zero=int((filt & (v == 0)).sum()),
                     median_v=float(np.median(v[filt])) if filt.any() else 0.0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    inside = shifted(inside0, s * dx, s * dy, False)
                    mq = shifted(tapmat, s * dx, s * dy, NOGEO)
                    counts = filt & inside & (mq == mat)
                    cq, Pq, nq, vq = shifted(c, s * dx, s * dy, 0), shifted(P, s * dx, s * dy, 0), shifted(ns, s * dx, s * dy, 0), shifted(v, s * dx, s * dy, 0)
                    dn = (ns[..., 0] * nq[..., 0] + ns[..., 1] * nq[..., 1]) + ns[..., 2] * nq[..., 2]
                    wn = np.maximum(dn, F(0))
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    d = Pq - P
                    dp = np.abs((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2])
                    wp = np.maximum(F(1) - dp * inv_plane, F(0))
                    dl = np.abs(luminance(cq) - lp)
                    wc = np.maximum(F(1) - dl * inv, F(0))
                    wt = ((HW[dy + 2] * HW[dx + 2]) * wn) * (wp * wc)
                    nx = sx + wt[..., None] * cq
                    nw = sw + wt
                    nv = svv + (wt * wt) * vq
                    for x in (dn, wn, d, dp, wp, dl, wc, wt, nx, nw, nv):
                        assert x.dtype == F
                    sx = np.where(counts[..., None], nx, sx); sw = np.where(counts, nw, sw); svv = np.where(counts, nv, svv)
                    if tally is not None:
                        t["counted"] += int(counts.sum())
                        t["wc0"] += int((counts & (wc == 0) & (wn > 0) & (wp > 0)).sum())
                        t["partial"] += int((counts & (wc > 0) & (wc < 1)).sum())
            den = np.where(filt, sw, F(1))
            res = sx / den[..., None]
            rv = svv / (den * den)
            assert res.dtype == F and rv.dtype == F
            c = np.where(filt[..., None], res, c); v = np.where(filt, rv, v)
            if tally is not None:
                tally.append(t)
        if flags & ALBEDO:
            mod = c * A
            assert mod.dtype == F
            c = np.where(filt[..., None], mod, c)
    out = np.empty((h, w, 4), F)
    out[..., :3], out[..., 3] = c, F(1)
    return out, int(filt.sum())


def level0(a, hb, guides, mguides=None, albedo=False):
    """(H, W, 2) float32 as rtx_debug_denoise_variance lays it out: (v, gv) of level 0, (0, 0) for a pixel that is not filterable"""
    a = np.ascontiguousarray(a, F)
    g = np.ascontiguousarray(guides, F)
    mat = g[..., 3].view(np.uint32)
    filt = (mat != NOGEO) & (a[..., 3] > 0)
    A = np.ascontiguousarray(mguides, F)[..., 0:3] if albedo else None
    _, v = variance_input(a, hb, A, filt)
    gv = prefilter(v, filt, mat, np.where(filt, mat, NOGEO))
    out = np.zeros(a.shape[:2] + (2,), F)
    out[..., 0], out[..., 1] = np.where(filt, v, F(0)), np.where(filt, gv, F(0))
    return out

"""The float32 emulator of rtx_denoise that tests/test_denoise.py holds the GPU to, bit for bit, the CPU test that its inputs are not vacuous, and the ABI without a device.

The filter is defined in include/rtx.h with + - * / abs max in a stated order and the library is built without contraction, so numpy float32 reproduces it to the bit:
    guides   Oracle.primary_rays (no jitter) -> trace_closest -> surface; a pixel that misses, whose material id is out of range or whose material has a Ke component > 0
             is "not filterable by geometry": material word 0xFFFFFFFF, P = n = 0
    colour   c = u1.xyz / max(u1.w, 1); a pixel is filterable when it is by geometry and u1.w > 0
    level i  step s = 1 << i; taps row-major over dy, dx = -2 .. 2; a tap counts inside the image, on a filterable pixel of the centre's material
The taps are visited one after the other for the whole image at once (a shifted view per tap), which is the sequential per-pixel order of the kernel.
"""
import ctypes as C
import functools
import os
import re

import numpy as np

import __graft_entry__ as graft

F = np.float32
NOGEO = np.uint32(0xFFFFFFFF)
MISS = np.uint32(0xFFFFFFFF)
# ---- the inputs of the GPU tests (tests/test_denoise.py) ----
W, H, ASPECT = 100, 50, 2.0
BASE = dict(width=W, height=H, sample_base=5, frame_seed=99, max_bounces=8, nee_samples=1)
SPP = 4
SIGMA_COLOR, SIGMA_PLANE, NORMAL_POWER_LOG2 = 0.5, 0.02, 5
LEVELS = (3, 5)
HW = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], F)


def guides_of(scene, width, height, aspect):
    """(H, W, 8) float32 as rtx_debug_denoise_guides lays them out: P3, material word (uint bits), n3, 0 — from the oracle alone"""
    rt, orc = graft.load_package(), graft.load_oracle()
    o = orc.Oracle().load(scene, aspect)
    rays = o.primary_rays(rt.Params(width=width, height=height, flags=0))
    hits = o.trace_closest(rays, 1)
    surf = o.surface(rays, hits)
    o.close()
    mats = np.asarray(scene.materials, F).reshape(-1, 32)
    mat = surf[:, 3].view(np.uint32)
    geo = (hits[:, 3].view(np.uint32) != MISS) & (mat < len(mats))
    geo[geo] = ~(mats[mat[geo], 8:11] > 0).any(1)
    g = np.zeros((width * height, 8), F)
    g[geo, 0:3], g[geo, 4:7] = surf[geo, 0:3], surf[geo, 4:7]
    g[:, 3].view(np.uint32)[:] = np.where(geo, mat, NOGEO)
    g = g.reshape(height, width, 8)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def cornell_guides(width=W, height=H, aspect=ASPECT):
    return guides_of(graft.load_package().Scene.cornell(), width, height, aspect)


@functools.lru_cache(maxsize=None)
def oracle_accum(flags, spp=SPP, sample_base=BASE["sample_base"], width=W, height=H, aspect=ASPECT):
    """the oracle's accumulation (H, W, 4) of the shared inputs; computed once per argument set and shared (read-only)"""
    rt, orc = graft.load_package(), graft.load_oracle()
    o = orc.Oracle().load(rt.Scene.cornell(), aspect)
    img, _ = o.render(rt.Params(**dict(BASE, width=width, height=height, spp=spp, flags=flags, sample_base=sample_base)))
    o.close()
    img.setflags(write=False)
    return img


def shifted(a, ox, oy, fill):
    """b[y, x] = a[y + oy, x + ox] where that lies inside, else fill"""
    h, w = a.shape[:2]
    b = np.full_like(a, fill)
    ys, xs = slice(max(0, -oy), min(h, h - oy)), slice(max(0, -ox), min(w, w - ox))
    yq, xq = slice(max(0, oy), min(h, h + oy)), slice(max(0, ox), min(w, w + ox))
    if ys.start < ys.stop and xs.start < xs.stop:
        b[ys, xs] = a[yq, xq]
    return b


def emulate(accum, guides, levels, sigma_color=SIGMA_COLOR, sigma_plane=SIGMA_PLANE, normal_power_log2=NORMAL_POWER_LOG2, tally=None):
    """-> (denoised (H, W, 4) float32, pixels filtered).  tally (optional): a list that receives per level a dict of how many taps of filterable centres each stop rejected"""
    a = np.ascontiguousarray(accum, F)
    g = np.ascontiguousarray(guides, F)
    h, w = a.shape[:2]
    cnt = np.maximum(a[..., 3], F(1))
    c = a[..., :3] / cnt[..., None]
    P, n, mat = g[..., 0:3], g[..., 4:7], g[..., 3].view(np.uint32)
    filt = (mat != NOGEO) & (a[..., 3] > 0)
    tapmat = np.where(filt, mat, NOGEO)                      # the word a tap is compared by: a pixel without samples counts for no neighbour
    inv_plane, inv_color = F(1.0) / F(sigma_plane), F(1.0) / F(sigma_color)
    inside0 = np.ones((h, w), bool)
    assert c.dtype == F and cnt.dtype == F and inv_plane.dtype == F and inv_color.dtype == F
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(levels):
            s = 1 << i
            isc = inv_color * F(s)
            sx = np.zeros((h, w, 3), F); sw = np.zeros((h, w), F)
            t = dict(outside=0, not_filterable=0, other_material=0, wn0=0, wp0=0, wc0=0, positive=0, counted=0)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    inside = shifted(inside0, s * dx, s * dy, False)
                    mq = shifted(tapmat, s * dx, s * dy, NOGEO)
                    counts = filt & inside & (mq == mat)
                    cq, Pq, nq = shifted(c, s * dx, s * dy, 0), shifted(P, s * dx, s * dy, 0), shifted(n, s * dx, s * dy, 0)
                    dn = (n[..., 0] * nq[..., 0] + n[..., 1] * nq[..., 1]) + n[..., 2] * nq[..., 2]
                    wn = np.maximum(dn, F(0))
                    for _ in range(normal_power_log2):
                        wn = wn * wn
                    d = Pq - P
                    dp = np.abs((n[..., 0] * d[..., 0] + n[..., 1] * d[..., 1]) + n[..., 2] * d[..., 2])
                    wp = np.maximum(F(1) - dp * inv_plane, F(0))
                    dc = (np.abs(cq[..., 0] - c[..., 0]) + np.abs(cq[..., 1] - c[..., 1])) + np.abs(cq[..., 2] - c[..., 2])
                    wc = np.maximum(F(1) - dc * isc, F(0))
                    wt = ((HW[dy + 2] * HW[dx + 2]) * wn) * (wp * wc)
                    for v in (dn, wn, d, dp, wp, dc, wc, wt, isc, cq):
                        assert v.dtype == F
                    nx = sx + wt[..., None] * cq
                    nw = sw + wt
                    assert nx.dtype == F and nw.dtype == F
                    sx = np.where(counts[..., None], nx, sx); sw = np.where(counts, nw, sw)
                    if tally is not None:
                        t["outside"] += int((filt & ~inside).sum())
                        t["not_filterable"] += int((filt & inside & (mq == NOGEO)).sum())
                        t["other_material"] += int((filt & inside & (mq != NOGEO) & (mq != mat)).sum())
                        # a stop rejects "on its own" where it alone is zero
                        t["wn0"] += int((counts & (wn == 0) & (wp > 0) & (wc > 0)).sum())
                        t["wp0"] += int((counts & (wp == 0) & (wn > 0) & (wc > 0)).sum())
                        t["wc0"] += int((counts & (wc == 0) & (wn > 0) & (wp > 0)).sum())
                        t["positive"] += int((counts & (wt > 0)).sum())
                        t["counted"] += int(counts.sum())
            res = sx / np.where(filt, sw, F(1))[..., None]
            assert res.dtype == F
            c = np.where(filt[..., None], res, c)
            if tally is not None:
                tally.append(t)
    out = np.empty((h, w, 4), F)
    out[..., :3], out[..., 3] = c, F(1)
    return out, int(filt.sum())


def tone_rmse(img, ref, mask):
    d = np.minimum(img[..., :3], F(1))[mask].astype(np.float64) - np.minimum(ref[..., :3], F(1))[mask].astype(np.float64)
    return float(np.sqrt((d * d).mean()))


def mean_of(accum):
    return accum[..., :3] / np.maximum(accum[..., 3:4], F(1))


def test_inputs_are_not_vacuous():
    """the GPU tests' exact inputs, on the oracle alone: every stop of the filter must reject taps on its own at every level, every level must have taps with weight,
    all three pixel classes must occur and nearly every filterable pixel must change — otherwise bit parity with the emulation would say nothing about that stop.  And the
    filter must help: the tone-mapped RMSE against the oracle's own 2048-spp image falls, for every flag word and level count of the tests"""
    g = cornell_guides()
    mat = g[..., 3].view(np.uint32)
    rt = graft.load_package()
    mats = np.asarray(rt.Scene.cornell().materials, F)
    a = oracle_accum(1)
    filt = (mat != NOGEO) & (a[..., 3] > 0)
    # classes: a miss and an emitter seen directly are both "not filterable by geometry"; tell them apart through the oracle once more
    orc = graft.load_oracle()
    o = orc.Oracle().load(rt.Scene.cornell(), ASPECT)
    rays = o.primary_rays(rt.Params(width=W, height=H, flags=0)); hits = o.trace_closest(rays, 1); surf = o.surface(rays, hits); o.close()
    hit = (hits[:, 3].view(np.uint32) != MISS).reshape(H, W)
    sm = surf[:, 3].view(np.uint32).reshape(H, W)
    emis = hit & (mat == NOGEO)
    assert (mats[sm[emis], 8:11] > 0).any(1).all()
    print(f"pixel classes: miss {int((~hit).sum())} / filterable {int(filt.sum())} / emissive {int(emis.sum())}; materials at first hit {len(set(mat[filt].tolist()))}")
    assert (~hit).any() and filt.any() and emis.any(), "all three pixel classes"
    assert len(set(mat[filt].tolist())) >= 2
    tally = []
    den3, nf = emulate(a, g, 3, tally=tally)
    assert nf == int(filt.sum())
    for i, t in enumerate(tally):
        print(f"level {i}: {t}")
        for k in ("outside", "not_filterable", "other_material", "wn0", "wp0", "wc0", "positive"):
            assert t[k] > 0, f"level {i}: the stop '{k}' rejects nothing on its own"
    changed = (den3[..., :3].view(np.uint32) != mean_of(a).view(np.uint32)).any(-1) & filt
    print(f"filterable pixels changed: {int(changed.sum())} of {int(filt.sum())}")
    assert changed.sum() > 0.95 * filt.sum()
    assert np.array_equal(den3[~filt][:, :3].view(np.uint32), mean_of(a)[~filt].view(np.uint32)), "a pass-through pixel's output is its input"
    for flags in (1, 3, 0):
        ref = mean_of(oracle_accum(flags, 2048, 1000))
        acc = oracle_accum(flags)
        f2 = (mat != NOGEO) & (acc[..., 3] > 0)
        raw = tone_rmse(mean_of(acc), ref, f2)
        for levels in LEVELS:
            den, _ = emulate(acc, g, levels)
            e = tone_rmse(den, ref, f2)
            print(f"flags {flags}, {SPP} spp: tone-mapped RMSE raw {raw:.4f}, denoised at levels {levels} {e:.4f}")
            assert e < raw, (flags, levels)


def test_abi_without_a_device():
    """the four entry points are exported and declared in rtx.h, and rtx_denoise(NULL, ...) is RTX_ERR_INVALID: fails before the feature, needs no GPU"""
    rt = graft.load_package()
    hdr = open(os.path.join(graft.ROOT, "include", "rtx.h")).read()
    for name in ("rtx_denoise", "rtx_read_denoised", "rtx_read_denoised_srgb8", "rtx_debug_denoise_guides"):
        assert hasattr(rt.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in rtx.h"
    assert "rtx_denoise_params" in hdr and "rtx_denoise_result" in hdr
    assert C.sizeof(rt.DenoiseParams) == 32 and C.sizeof(rt.DenoiseResult) == 32
    assert rt.lib.rtx_denoise(None, 8, 8, None, None) == -1
    assert rt.lib.rtx_read_denoised(None, None, 0) == -1 and rt.lib.rtx_read_denoised_srgb8(None, None, 0) == -1 and rt.lib.rtx_debug_denoise_guides(None, 8, 8, None) == -1

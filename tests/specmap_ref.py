"""numpy emulation of the specular, roughness and metalness maps as include/rtx.h defines them (SPECULAR MAPS): Ks', Pr', Pm' per hit from texture_ref's taps and tables and
the package's half_round, the rows-first look-up of the energy table, the row arithmetic of the host header (csrc/rtx_specmap_host.hpp) and the loader's zero-scalar rule.
float32 throughout, one numpy operation per written operation.  Shared by tests/test_specmap_ref.py (its own properties, no GPU) and tests/test_specmap.py (the device is
held to it bit for bit)."""
import numpy as np

import texture_ref as tr

F = np.float32
NO_TEX = np.uint32(0xFFFFFFFF)
MAP_KS, MAP_PR, MAP_PM = 6, 8, 10


def channel(rgba8, k, s, t):
    """the bilinear value of T_linear[byte k] of the four taps of Sample (k = 1: green = roughness, k = 2: blue = metalness) -> (n,) float32"""
    px = np.asarray(rgba8, np.uint8)
    T = tr.table(False)
    ix0, ix1, iy0, iy1, fx, fy = tr.taps(px.shape, s, t)
    c00, c10, c01, c11 = T[px[iy0, ix0, k]], T[px[iy0, ix1, k]], T[px[iy1, ix0, k]], T[px[iy1, ix1, k]]
    top = c00 + fx * (c10 - c00)
    bot = c01 + fx * (c11 - c01)
    out = top + fy * (bot - top)
    assert out.dtype == np.float32
    return out


def table_values(half_round, materials):
    """the device's material table: (Ks (n, 3), Pr (n,), Pm (n,)) = half_round of the 128-byte records' fields"""
    m = np.asarray(materials, np.float32).reshape(-1, 32)
    return tr.half_round_array(half_round, m[:, 4:7]), tr.half_round_array(half_round, m[:, 12]), tr.half_round_array(half_round, m[:, 13])


def ks_prime(half_round, ks_table, rgba8, srgb, s, t):
    """Ks'[k] = half_round(m.Ks[k] * Sample(tex, s, t)[k]); ks_table: (3,) or (n, 3), the TABLE's (rounded) values"""
    return tr.half_round_array(half_round, np.asarray(ks_table, np.float32) * tr.sample(rgba8, srgb, s, t))


def pr_prime(half_round, pr_table, rgba8, s, t):
    """Pr' = half_round(m.Pr * g), g from the green byte through the linear table"""
    return tr.half_round_array(half_round, np.asarray(pr_table, np.float32) * channel(rgba8, 1, s, t))


def pm_prime(half_round, pm_table, rgba8, s, t):
    """Pm' = half_round(m.Pm * b), b from the blue byte through the linear table"""
    return tr.half_round_array(half_round, np.asarray(pm_table, np.float32) * channel(rgba8, 2, s, t))


def specular_probe(half_round, textures, maps, materials, emits, tri_mat, tri_uv3, hits):
    """rtx_debug_specular: textures = [(rgba8, srgb)], maps = (ks, pr, pm) lists per material (-1 = none), materials (n, 32), emits (n,) bool (the device's emitter test),
    tri_mat / tri_uv3 per global triangle id, hits (n, 4) -> ((n, 5) float32, (n, 3) uint32)"""
    hits = np.asarray(hits, np.float32).reshape(-1, 4)
    prim = hits[:, 3].copy().view(np.uint32)
    hit = prim != NO_TEX
    ks_t, pr_t, pm_t = table_values(half_round, materials)
    val = np.zeros((len(hits), 5), np.float32); ids = np.full((len(hits), 3), NO_TEX, np.uint32)
    p = np.where(hit, prim, 0).astype(np.int64)
    mat = np.asarray(tri_mat)[p].astype(np.int64)
    val[hit, :3] = ks_t[mat[hit]]; val[hit, 3] = pr_t[mat[hit]]; val[hit, 4] = pm_t[mat[hit]]
    s, t = tr.interp_uv(np.asarray(tri_uv3, np.float32)[p], hits[:, 1], hits[:, 2])
    shaded = hit & ~np.asarray(emits, bool)[mat]
    for slot, lst in enumerate(maps):
        tex_of = np.array([(-1 if x is None else x) for x in lst] + [-1] * (len(ks_t) - len(lst)), np.int64)[mat]
        for tex in np.unique(tex_of[shaded & (tex_of >= 0)]):
            sel = shaded & (tex_of == tex)
            px, srgb = textures[tex]
            ids[sel, slot] = tex
            if slot == 0:
                val[sel, :3] = ks_prime(half_round, ks_t[mat[sel]], px, srgb, s[sel], t[sel])
            elif slot == 1:
                val[sel, 3] = pr_prime(half_round, pr_t[mat[sel]], px, s[sel], t[sel])
            else:
                val[sel, 4] = pm_prime(half_round, pm_t[mat[sel]], px, s[sel], t[sel])
    return val, ids


def ess_rows(pr, rows):
    """fr = Pr' * (float)(rows - 1);  r0 = clamp((int)floorf(fr), 0, rows - 1);  r1 = min(r0 + 1, rows - 1);  wr = fr - (float)r0"""
    pr = np.asarray(pr, np.float32)
    fr = pr * F(rows - 1)
    r0 = np.clip(np.floor(fr), 0, rows - 1).astype(np.int64)
    r1 = np.minimum(r0 + 1, rows - 1)
    wr = fr - r0.astype(np.float32)
    assert wr.dtype == np.float32
    return r0, r1, wr


def ndotv_taps(ndotv):
    """i0, i1, w of ess_lut: NdotV saturated, f = NdotV * 15.0f, i0 = (int)floorf(f), i1 = min(i0 + 1, 15), w = f - (float)i0"""
    x = np.asarray(ndotv, np.float32)
    x = np.minimum(np.maximum(x, F(0.0)), F(1.0))
    f = x * F(15.0)
    i0 = np.floor(f).astype(np.int64)
    i1 = np.minimum(i0 + 1, 15)
    w = f - i0.astype(np.float32)
    return i0, i1, w


def ess_lut(lut16, ndotv):
    """the material's own look-up: v0 + w * (v1 - v0); lut16: (16,) or (n, 16)"""
    L = np.asarray(lut16, np.float32)
    i0, i1, w = ndotv_taps(ndotv)
    if L.ndim == 1:
        v0, v1 = L[i0], L[i1]
    else:
        k = np.arange(len(i0)); v0, v1 = L[k, i0], L[k, i1]
    return v0 + w * (v1 - v0)


def ess_table(table, pr, ndotv):
    """the energy table's look-up, rows first: L[i] = A[r0][i] + wr * (A[r1][i] - A[r0][i]) for i = i0, i1;  Ess = L[i0] + w * (L[i1] - L[i0])"""
    A = np.asarray(table, np.float32).reshape(-1, 16)
    r0, r1, wr = ess_rows(pr, len(A))
    i0, i1, w = ndotv_taps(ndotv)
    L0 = A[r0, i0] + wr * (A[r1, i0] - A[r0, i0])
    L1 = A[r0, i1] + wr * (A[r1, i1] - A[r0, i1])
    out = L0 + w * (L1 - L0)
    assert out.dtype == np.float32
    return out


def blend_row(table, pr):
    """the LUT of the material that equals a constant roughness map Pr' under the table: LUT[i] = A[r0][i] + wr * (A[r1][i] - A[r0][i]) for all 16 i -> (16,) float32"""
    A = np.asarray(table, np.float32).reshape(-1, 16)
    r0, r1, wr = ess_rows(np.array([pr], np.float32), len(A))
    return (A[r0[0]] + wr[0] * (A[r1[0]] - A[r0[0]])).astype(np.float32)


def table_error(table, rows):
    """rtx_set_ess_table's argument check as csrc/rtx_specmap_host.hpp words it: None = valid"""
    if table is None and rows == 0:
        return None
    if table is None:
        return "set_ess_table: null table with a row count"
    if rows < 2 or rows > 256:
        return "set_ess_table: rows must be in [2, 256] (or NULL / 0 to clear)"
    if not np.isfinite(np.asarray(table, np.float32).ravel()[:rows * 16]).all():
        return "set_ess_table: non-finite value"
    return None


def zero_scalar_rule(rec5):
    """(Ks.xyz, Pr, Pm) after the loader's rule with every map bound -> (values, (ks, pr, pm) changed flags)"""
    r = np.array(rec5, np.float32)
    ck = bool((r[:3] == 0).all()); cr = bool(r[3] == 0); cm = bool(r[4] == 0)
    if ck:
        r[:3] = 1
    if cr:
        r[3] = 1
    if cm:
        r[4] = 1
    return r, (ck, cr, cm)

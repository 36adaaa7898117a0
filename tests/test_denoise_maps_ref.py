"""rtx_denoise's map guides without a GPU: the ABI, that the inputs of tests/test_denoise_maps.py are not vacuous, and that the twin (tests/denoise_maps_ref.py) keeps what the
extension exists to keep — an image whose only detail is the albedo's comes out of flag 1 as it went in, and does not come out of flag 0 that way."""
import ctypes as C
import os
import re

import numpy as np

import __graft_entry__ as graft
import denoise_maps_ref as mr
from denoise_maps_ref import F, NOGEO


def test_abi_without_a_device():
    """fails before the feature: the flag names, the entry point and its NULL-context error"""
    rt = graft.load_package()
    hdr = open(os.path.join(graft.ROOT, "include", "rtx.h")).read()
    assert re.search(r"\bint\s+rtx_debug_denoise_map_guides\s*\(", hdr), "rtx_debug_denoise_map_guides is not declared in rtx.h"
    assert re.search(r"#define\s+RTX_DENOISE_ALBEDO\s+1u\b", hdr) and re.search(r"#define\s+RTX_DENOISE_MAPPED_NORMALS\s+2u\b", hdr)
    assert re.search(r"uint32_t\s+flags;[^\n]*\n\s*uint32_t\s+reserved\[3\];", hdr), "rtx_denoise_params: flags, then three reserved words"
    assert hasattr(rt.lib, "rtx_debug_denoise_map_guides")
    assert rt.DENOISE_ALBEDO == 1 and rt.DENOISE_MAPPED_NORMALS == 2
    assert C.sizeof(rt.DenoiseParams) == 32 and [f[0] for f in rt.DenoiseParams._fields_] == ["levels", "normal_power_log2", "sigma_color", "sigma_plane", "reserved"]
    assert rt.lib.rtx_debug_denoise_map_guides(None, 8, 8, None) == -1


def test_inputs_are_not_vacuous():
    """the KD variant on the oracle's first hits: both extensions have something to do at the three sizes' largest, or bit parity with the twin would say nothing"""
    _, _, g, mg = mr.oracle_inputs("KD")
    tab = mr.Tables(mr.variant("KD"))
    mat = g[..., 3].view(np.uint32)
    geo = mat != NOGEO
    seen = sorted(set(mat[geo].tolist()))
    mapped = [m for m in seen if tab.kd_maps[m] >= 0]
    print(f"materials at first hit {seen}, with a map_Kd {mapped}; not filterable by geometry {int((~geo).sum())} of {geo.size} pixels")
    assert len(mapped) >= 2 and (~geo).any()
    A, nm, n = mg[..., 0:3], mg[..., 4:7], g[..., 4:7]
    at_floor, above = geo & (A == mr.FLOOR).any(-1), geo & (A > mr.FLOOR).all(-1)
    print(f"pixels with a channel at the floor {int(at_floor.sum())}, with every channel above it {int(above.sum())}")
    assert at_floor.any() and above.any()
    assert (A[~geo] == 1).all() and not nm[~geo].any()
    differs = geo & (nm.view(np.uint32) != n.view(np.uint32)).any(-1)
    print(f"nm != n at {int(differs.sum())} pixels, nm == n at {int((geo & ~differs).sum())}")
    assert differs.any() and (geo & ~differs).any()
    tally = []
    a = mr.synthetic_accum(mg)
    mr.emulate_maps(a, g, mg, 5, mr.MAPPED_NORMALS, tally=tally)
    for i, t in enumerate(tally):
        print(f"level {i}: {t}")
        assert t["wn_lower"] > 0, f"level {i}: no tap's normal stop is tighter under the mapped normals"
    # ... and flag 2 with nm = n is the filter as it was, to the bit (the copy of the tap loop is a copy)
    mg0 = np.array(mg, F, copy=True); mg0[..., 4:7] = n
    rng = np.random.default_rng(1)
    noisy = a.copy(); noisy[..., :3] *= rng.uniform(0.5, 1.5, a.shape[:2] + (3,)).astype(F)
    for flags in (0, 1):
        assert np.array_equal(mr.emulate_maps(noisy, g, mg0, 3, flags | mr.MAPPED_NORMALS)[0].view(np.uint32), mr.emulate_maps(noisy, g, mg0, 3, flags)[0].view(np.uint32))


def test_the_filter_keeps_albedo_detail():
    """u1 = A * L with a constant L: flag 1 returns u1 within rounding — one product, two divisions, per level a 25-term weighted mean of values within 2 ulp of L, one product:
    relative 2^-18 — at every pixel; flag 0 moves filterable pixels of mapped materials by more than 5 % (the share is printed: recorded, not fixed in advance)"""
    _, _, g, mg = mr.oracle_inputs("KD")
    a = mr.synthetic_accum(mg)
    d1, nf = mr.emulate_maps(a, g, mg, 5, mr.ALBEDO)
    e1 = mr.rel_err(d1, a)
    print(f"flag 1: largest relative error {e1.max():.3e} (bound {mr.REL:.3e}) over {a.shape[0] * a.shape[1]} pixels, {nf} filtered")
    assert (e1 <= mr.REL).all()
    moved, mapped = mr.moved_under_flag0("KD")
    print(f"flag 0: {int(moved.sum())} of {int(mapped.sum())} filterable pixels of mapped materials move by more than 5 % ({100.0 * moved.sum() / mapped.sum():.1f} %)")
    assert moved.sum() > 0
    ys, xs = np.nonzero(moved)
    print("the first of them (y, x):", list(zip(ys[:8].tolist(), xs[:8].tolist())))

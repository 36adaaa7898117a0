"""rtx_denoise_variance without a device: the ABI, that the inputs of tests/test_denoise_var.py are not vacuous, and the quality condition the feature exists for — all on the
oracle's per-sample frames through tests/test_adaptive_ref.py's emulation (the Cornell box at 100 x 50; min 4, step 4, max 16 spp, threshold 0.25) and the float32 twin of
tests/denoise_var_ref.py."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import __graft_entry__ as graft
import denoise_var_ref as vr
import test_adaptive_ref as ar
import test_denoise_ref as ref
from test_denoise_ref import F

FLAGS, LEVELS = (1, 3, 0), (1, 3, 5)
CASES = [(flags, tile) for flags in FLAGS for tile in ar.TILES]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def state(flags, tile):
    """(u1, half) of the adaptive emulation (denoise_var_ref.Emulation: `half` is the sum of the odd sample ids, as on the device), read-only and shared"""
    e, _ = vr.emulate(flags, tile)
    return e.accum, e.half


@pytest.mark.parametrize("flags,tile", CASES)
def test_the_odd_half_changes_nothing_but_half(flags, tile):
    """denoise_var_ref.Emulation against tests/test_adaptive_ref.py's, whose `half` holds the EVEN sample ids at the tests' odd sample_base: u1, the counts, the flags and
    the result are the same to the bit, the two halves add up to u1 within rounding, and they differ"""
    e, res = vr.emulate(flags, tile)
    o, want = ar.emulate(flags, tile)
    assert res == want and np.array_equal(e.count, o.count) and np.array_equal(e.flag, o.flag) and e.converged_after_pass == o.converged_after_pass
    assert np.array_equal(bits(e.accum), bits(o.accum)) and np.array_equal(bits(e.half[..., 3]), bits(o.half[..., 3]))
    assert not np.array_equal(bits(e.half), bits(o.half))
    assert np.allclose(e.half[..., :3].astype(np.float64) + o.half[..., :3], e.accum[..., :3], rtol=1e-5, atol=1e-6)
    # the odd ids, summed in sample order, of a pixel that took all 16 samples and of one that stopped at 4
    fr = ar.oracle_frames(flags)
    for n in (ar.MAX_SPP, ar.MIN_SPP):
        ys, xs = np.nonzero(e.accum[..., 3] == n)
        assert len(ys), n
        y, x = int(ys[0]), int(xs[0])
        s = np.zeros(3, F)
        for k in range(n):
            if (ar.BASE["sample_base"] + k) & 1:
                s = s + fr[k][y, x, :3]
        assert np.array_equal(bits(s), bits(e.half[y, x, :3])), (n, y, x)


def test_abi_without_a_device():
    """the three entry points are exported and declared in rtx.h, the struct has 32 bytes and rtx_denoise_variance(NULL, ...) is RTX_ERR_INVALID: fails before the feature"""
    rt = graft.load_package()
    hdr = open(os.path.join(graft.ROOT, "include", "rtx.h")).read()
    for name in ("rtx_denoise_variance", "rtx_read_adaptive_half", "rtx_debug_denoise_variance"):
        assert hasattr(rt.lib, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name + " is not declared in rtx.h"
    assert "rtx_denoise_var_params" in hdr
    assert C.sizeof(rt.DenoiseVarParams) == 32 and C.sizeof(rt.DenoiseParams) == 32
    assert rt.lib.rtx_denoise_variance(None, 8, 8, None, None) == -1
    assert rt.lib.rtx_read_adaptive_half(None, None, 0) == -1 and rt.lib.rtx_debug_denoise_variance(None, 8, 8, 0, None) == -1


def test_cli_usage_errors():
    """--denoise-variance without --adaptive, or on several GPUs, and --sigma-var without it, exit with status 2 before any device is touched"""
    graft.load_package()
    exe = os.path.join(graft.PKG_DIR, "rtx_render")
    for args in (["--denoise-variance"], ["--denoise-variance", "--gpus", "2"], ["--adaptive", "0.25", "--denoise-variance", "--gpus", "2"], ["--adaptive", "0.25", "--sigma-var", "4"]):
        r = subprocess.run([exe, "--scene", "cornell"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and ("--denoise-variance" in r.stderr or "--adaptive" in r.stderr), (args, r.returncode, r.stderr[-300:])
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--denoise-variance" in r.stdout and "--sigma-var" in r.stdout


@pytest.mark.parametrize("flags,tile", CASES)
def test_inputs_are_not_vacuous(flags, tile):
    """at every level the colour stop alone rejects taps and weights others partially, the prefilter changes v on most filterable pixels, some pixels have v == 0 (their
    halves agree: the 2^-20 of the definition is exercised), the variance falls from level to level, and pass-through pixels come out as they went in"""
    a, hb = state(flags, tile)
    g = ref.cornell_guides()
    tally = []
    den, nf = vr.emulate_var(a, hb, g, None, 5, tally=tally)
    filt = vr.filterable(a, g)
    assert nf == int(filt.sum()) and 0 < nf < a.shape[0] * a.shape[1]
    for i, t in enumerate(tally):
        print(f"flags {flags} tile {tile} level {i}: {t}")
        assert t["wc0"] > 0, f"level {i}: the colour stop rejects nothing on its own"
        assert t["partial"] > 0, f"level {i}: no tap with 0 < wc < 1"
        assert t["gv_ne_v"] > 0.5 * t["filterable"], f"level {i}: the prefilter changes too few pixels"
        if i:
            assert t["median_v"] < tally[i - 1]["median_v"], f"level {i}: the median variance does not fall"
    assert 0 < tally[0]["v_zero"] < 0.05 * nf, "level 0: pixels whose halves agree exist and are few"
    assert np.array_equal(bits(den[..., :3])[~filt], bits(ref.mean_of(a))[~filt]), "a pass-through pixel's output is its input"
    assert (den[..., 3] == 1).all()
    lv = vr.level0(a, hb, g)
    assert not lv[~filt].any() and (lv[filt] >= 0).all()


@pytest.mark.parametrize("flags,tile", CASES)
def test_quality_condition(flags, tile):
    """tone-mapped RMSE against the oracle's own 2048-spp image: variance-guided < rtx_denoise's defaults < raw, at 1, 3 and 5 levels"""
    a, hb = state(flags, tile)
    g = ref.cornell_guides()
    filt = vr.filterable(a, g)
    want = ref.mean_of(ref.oracle_accum(flags, 2048, 1000))
    raw = ref.tone_rmse(ref.mean_of(a), want, filt)
    for levels in LEVELS:
        e_var = ref.tone_rmse(vr.emulate_var(a, hb, g, None, levels)[0], want, filt)
        e_dn = ref.tone_rmse(ref.emulate(a, g, levels)[0], want, filt)
        print(f"flags {flags} tile {tile} levels {levels}: raw {raw:.4f}, rtx_denoise {e_dn:.4f}, variance-guided {e_var:.4f}")
        assert e_var < e_dn < raw, (flags, tile, levels)

#!/usr/bin/env python3
"""What rtx_denoise_variance buys, from the numpy twins and the CPU oracle alone (no GPU); writes a markdown report.

The Cornell box at 100 x 50 through tests/test_adaptive_ref.py's emulation (per-sample oracle frames); the metric is tests/test_denoise_ref.py's tone_rmse over the filterable
pixels against the oracle's own 2048-spp image.  Table 1: the adaptive frame of the tests (min 4, step 4, max 16 spp, threshold 0.25), raw / rtx_denoise's defaults /
variance-guided at sigma_var 4, levels 1, 3, 5.  Table 2: uniform 4 and 16 spp (threshold 0), the best constant sigma_color of {0.25, 0.5, 1.0} against a sweep of sigma_var.
    python tools/denoise_var_quality.py [--out profiles/denoise_var_quality.md]"""
import argparse, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import denoise_var_ref as vr
import test_adaptive_ref as ar
import test_denoise_ref as ref

LEVELS, FLAGS, SWEEP, COLORS = (1, 3, 5), (1, 3, 0), (1.0, 2.0, 4.0, 8.0, 16.0), (0.25, 0.5, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    g = ref.cornell_guides()
    want = {fl: ref.mean_of(ref.oracle_accum(fl, 2048, 1000)) for fl in FLAGS}
    out = ["# rtx_denoise_variance: what the variance-guided colour stop buys", "",
           "From `tools/denoise_var_quality.py`: the committed numpy twins (`tests/test_denoise_ref.py`, `tests/denoise_var_ref.py`) on the CPU oracle's per-sample frames of the",
           "Cornell box at 100 x 50 (`tests/test_adaptive_ref.py`, with `half` as the device keeps it: `denoise_var_ref.Emulation`); tone-mapped RMSE over the filterable pixels against the oracle's own 2048-spp image.  Lower is better.", "",
           "## The adaptive frame of the tests (min 4, step 4, max 16 spp, threshold 0.25)", "",
           "| flags / tile | raw | `rtx_denoise` defaults, levels 1 / 3 / 5 | variance-guided, sigma_var 4, levels 1 / 3 / 5 |", "|---|---|---|---|"]
    for fl in FLAGS:
        for ts in ar.TILES:
            e, _ = vr.emulate(fl, ts)
            filt = vr.filterable(e.accum, g)
            raw = ref.tone_rmse(ref.mean_of(e.accum), want[fl], filt)
            dn = [ref.tone_rmse(ref.emulate(e.accum, g, lv)[0], want[fl], filt) for lv in LEVELS]
            dv = [ref.tone_rmse(vr.emulate_var(e.accum, e.half, g, None, lv)[0], want[fl], filt) for lv in LEVELS]
            out.append(f"| {fl} / {ts} | {raw:.4f} | " + " / ".join(f"{x:.4f}" for x in dn) + " | " + " / ".join(f"{x:.4f}" for x in dv) + " |")
    out += ["", "## Uniform sampling (threshold 0, tile 16), 5 levels: the best constant sigma_color of {0.25, 0.5, 1.0} against sigma_var", "",
            "| flags / spp | raw | best constant (its sigma_color) | " + " | ".join(f"sigma_var {s:g}" for s in SWEEP) + " |", "|---|---|---|" + "---|" * len(SWEEP)]
    for fl in FLAGS:
        for spp in (4, 16):
            e, _ = vr.emulate(fl, 16, max_spp=spp, threshold=0.0)
            filt = vr.filterable(e.accum, g)
            raw = ref.tone_rmse(ref.mean_of(e.accum), want[fl], filt)
            best = min((ref.tone_rmse(ref.emulate(e.accum, g, 5, sigma_color=sc)[0], want[fl], filt), sc) for sc in COLORS)
            sw = [ref.tone_rmse(vr.emulate_var(e.accum, e.half, g, None, 5, sigma_var=s)[0], want[fl], filt) for s in SWEEP]
            out.append(f"| {fl} / {spp} | {raw:.4f} | {best[0]:.4f} ({best[1]:g}) | " + " | ".join(f"{x:.4f}" for x in sw) + " |")
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()

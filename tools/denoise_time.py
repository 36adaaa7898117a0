#!/usr/bin/env python3
"""What rtx_denoise costs, measured on the GPU with RTX_OPT_KERNEL_TIMING; writes a markdown report.

Per scene (the headline Cornell frame, 64 spp; the Sponza-class atrium, 16 spp; both 1920 x 1080): the frame's own render_ms, then rtx_denoise with levels = 1 .. 5 under
RTX_OPT_DENOISE_LDS_STEP 0 (every level direct) and 4 (steps 1, 2 and 4 staged in LDS), the two forms ALTERNATING round by round in one process on one device.
rtx_denoise_result reports the guides and the filter as two hipEvent intervals, so the time of level i is filter_ms(levels = i + 1) - filter_ms(levels = i) of the same
form: the last level writes the denoised image instead of a ping-pong image, the same bytes.  Bytes model per level and pixel: 16 B colour + 32 B guides read once + 16 B
written = 64 B; the fraction is that traffic per measured time against the 6.3 TB/s a float4 copy achieves on this part.
    python tools/denoise_time.py [--rounds 5] [--out profiles/denoise_time.md]"""
import argparse, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--out", default="")
args = ap.parse_args()
W, H, LEVELS = 1920, 1080, 5
HBM_ACHIEVABLE = 6.3e12           # B/s, float4 copy
FORMS = ((0, "direct"), (4, "LDS-staged"))
med = statistics.median


def main():
    import __graft_entry__ as g
    rt = g.load_package()
    out = ["# rtx_denoise: time per level, LDS-staged against direct", "",
           f"One MI355X, {W} x {H}, RTX_OPT_KERNEL_TIMING (hipEvent intervals around the guides kernel and around the level kernels), {args.rounds} rounds, the two forms alternating",
           "round by round in one process; medians (min .. max).  Level i has step 1 << i; its time is filter_ms(levels = i + 1) - filter_ms(levels = i) of the same form and round.",
           f"Bytes model: 64 B per pixel and level (16 colour + 32 guides read once, 16 written) = {W * H * 64 / 1e6:.1f} MB; fraction = model bytes / time / 6.3 TB/s (float4 copy).", ""]
    for name, scene, spp in (("Cornell box (headline frame, 64 spp)", rt.Scene.cornell(), 64), ("Sponza-class atrium (262 144 triangles, 16 spp)", rt.Scene.sponza_class(), 16)):
        c = rt.Context(0)
        c.set_option(rt.OPT_KERNEL_TIMING, 1)
        c.upload(scene, W / H)
        p = rt.Params(width=W, height=H, spp=spp, max_bounces=8, nee_samples=1, flags=1)
        frames = []
        for _ in range(3):
            c.clear(W, H); c.render(p); frames.append(c.stats().render_ms)
        frame_ms = med(frames[1:])
        guides, filt = [], {f: [[] for _ in range(LEVELS + 1)] for f, _ in FORMS}
        for f, _ in FORMS:                                          # warm-up: code objects, buffers
            c.set_option(rt.OPT_DENOISE_LDS_STEP, f); c.denoise(W, H, LEVELS)
        for rnd in range(args.rounds):
            for f, _ in (FORMS if rnd % 2 == 0 else FORMS[::-1]):
                c.set_option(rt.OPT_DENOISE_LDS_STEP, f)
                for lv in range(1, LEVELS + 1):
                    r = c.denoise(W, H, lv)
                    filt[f][lv].append(r.filter_ms); guides.append(r.guides_ms)
        res = c.denoise(W, H, LEVELS)
        out += [f"## {name}", "", f"frame (rtx_render, render_ms): {frame_ms:.3f} ms; guides: {med(guides):.4f} ms ({min(guides):.4f} .. {max(guides):.4f}); "
                f"{res.pixels_filtered} pixels filtered, {res.pixels_passed} passed through", "",
                "| level | step | direct ms | fraction of 6.3 TB/s | LDS-staged ms | fraction of 6.3 TB/s |", "|---|---|---|---|---|---|"]
        model = W * H * 64
        best_total = 0.0
        for lv in range(LEVELS):
            cells, t = [], {}
            for f, _ in FORMS:
                if f and (1 << lv) > f:
                    cells += ["(direct)", ""]; continue
                prev = filt[f][lv] if lv else [0.0] * args.rounds
                d = [a - b for a, b in zip(filt[f][lv + 1], prev)]
                t[f] = med(d)
                cells += [f"{med(d):.4f} ({min(d):.4f} .. {max(d):.4f})", f"{model / (med(d) * 1e-3) / HBM_ACHIEVABLE:.2f}" if med(d) > 0 else "-"]
            best_total += min(t.values())
            out.append(f"| {lv} | {1 << lv} | " + " | ".join(cells) + " |")
        td, ts = filt[0][LEVELS], filt[4][LEVELS]
        out.append(f"| all {LEVELS} | | {med(td):.4f} ({min(td):.4f} .. {max(td):.4f}) | {LEVELS * model / (med(td) * 1e-3) / HBM_ACHIEVABLE:.2f} | "
                   f"{med(ts):.4f} ({min(ts):.4f} .. {max(ts):.4f}), steps 8 and 16 direct | {LEVELS * model / (med(ts) * 1e-3) / HBM_ACHIEVABLE:.2f} |")
        c.set_option(rt.OPT_DENOISE_LDS_STEP, 4)
        d2 = [c.denoise(W, H, LEVELS) for _ in range(args.rounds + 1)][1:]
        tot2 = med([r.filter_ms + r.guides_ms for r in d2])
        out += ["", f"Default (RTX_OPT_DENOISE_LDS_STEP 4), guides + {LEVELS} levels: {tot2:.4f} ms = {100 * tot2 / frame_ms:.2f} % of the frame's {frame_ms:.3f} ms "
                f"({100 * tot2 / (frame_ms / spp):.1f} % of one sample per pixel); the faster form of every level summed: {best_total:.4f} ms.", ""]
        c.close()
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()

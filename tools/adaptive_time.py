#!/usr/bin/env python3
"""What adaptive sampling (rtx_render_adaptive) costs and buys, measured on the GPU; writes a markdown report.

1. THE DEFAULT PATH HAS NOT SLOWED: the headline frame (Cornell, 1080p, 64 spp) and one general-path frame (Sponza class, 1080p, 16 spp) through plain rtx_render,
   alternating between this tree's library and the parent commit's (--parent-pkg: the parent's royaltracer-dx_amd directory with its library built; one process holds one
   library, so every measurement is a child process).  Passes if the difference of the medians lies inside the spread of the parent's own repeated runs of the session.
2. WHAT THE FEATURE BUYS (reporting only): Cornell at 1080p, cap 64: wall time and pixel-samples of render_adaptive at a few thresholds and its RMSE against a 1 024-spp
   image, beside rtx_render at 64 spp; threshold 0 against plain rtx_render = the per-pass cost (criterion, list, read-back).
Every GPU step is a child process under its own `timeout`; the first one that fails ends the run.
    python tools/adaptive_time.py --parent-pkg DIR/royaltracer-dx_amd [--rounds 3] [--out profiles/adaptive_time.md]"""
import argparse, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-pkg", default="")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--out", default="")
ap.add_argument("--child", default="", help="(child process) frame:cornell | frame:sponza | adaptive")
ap.add_argument("--pkg", default="", help="(child process) package directory to load instead of this tree's")
args = ap.parse_args()
W, H, CAP = 1920, 1080, 64
THRESHOLDS = (0.05, 0.1, 0.2, 0.4)


def wall_ms(fn, reps):
    """host clock around calls that return with the stream drained"""
    out = []
    for _ in range(reps):
        t = time.perf_counter(); fn(); out.append((time.perf_counter() - t) * 1e3)
    return out


def child():
    import numpy as np
    import __graft_entry__ as g
    if args.pkg:
        g.PKG_DIR = os.path.abspath(args.pkg)
    rt = g.load_package()
    c = rt.Context(0)
    if args.child.startswith("frame:"):
        kind = args.child.split(":")[1]
        sc = rt.Scene.cornell() if kind == "cornell" else rt.Scene.sponza_class()
        c.upload(sc, W / H)
        p = rt.Params(width=W, height=H, spp=CAP if kind == "cornell" else 16, max_bounces=8, nee_samples=1, flags=1)
        def frame():
            c.clear(W, H); c.render(p)
        frame(); frame()                                          # warm-up: code objects, buffers, launch-size predictions
        ms = wall_ms(frame, 9 if kind == "cornell" else 5)
        print("RESULT " + json.dumps(dict(kind=kind, lib=rt.LIB_PATH, ms=ms, device_ms=c.stats().render_ms)))
    else:
        c.upload(rt.Scene.cornell(), W / H)
        base = dict(width=W, height=H, max_bounces=8, nee_samples=1, flags=1)
        c.clear(W, H)
        for k in range(16):                                       # the 1 024-spp image, ids far from the ones measured below
            c.render(rt.Params(spp=64, sample_base=100001 + 64 * k, **base))
        a = c.read_accum(); truth = a[..., :3] / np.maximum(a[..., 3:], 1.0)
        def rmse(img):
            return float(np.sqrt(np.mean((img[..., :3] / np.maximum(img[..., 3:], 1.0) - truth) ** 2)))
        p = rt.Params(spp=CAP, **base)
        def plain():
            c.clear(W, H); c.render(p)
        plain(); plain()
        rows = [dict(what="rtx_render 64 spp", ms=wall_ms(plain, 7), samples=c.stats().paths, passes=1, rmse=rmse(c.read_accum()))]
        for thr in (0.0,) + THRESHOLDS:
            res = [None]
            def adaptive():
                c.clear(W, H); res[0] = c.render_adaptive(p, 8, 8, CAP, thr)
            adaptive(); adaptive()
            ms = wall_ms(adaptive, 7)
            r = res[0]
            rows.append(dict(what=f"render_adaptive threshold {thr:g}", ms=ms, samples=r.pixel_samples, passes=r.passes, converged=r.chunks_converged, at_max=r.chunks_at_max,
                             chunks=r.chunks, rmse=rmse(c.read_accum())))
        print("RESULT " + json.dumps(rows))
    c.close()


def run_child(what, pkg, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", what] + (["--pkg", pkg] if pkg else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=dict(os.environ, RTX_NO_TORCH_PRELOAD="1"))
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
        sys.exit(f"step `{what}` ({pkg or 'this tree'}) ended with status {r.returncode}: nothing more is started")
    return json.loads(line[0][7:])


def main():
    if not args.parent_pkg:
        sys.exit("--parent-pkg is needed: the parent commit's royaltracer-dx_amd directory with librtx_hip.so built")
    med = statistics.median
    out = ["# Adaptive sampling: what it costs and what it buys", "",
           f"MI355X, 1920 x 1080, wall time around calls that return with the stream drained (clear + render), two warm-up calls per process; one process per row and library.", ""]
    out += ["## The default path: plain rtx_render, this library against the parent commit's, alternating", "",
            "| frame | round | parent ms (median; min .. max) | this ms (median; min .. max) |", "|---|---|---|---|"]
    verdicts = []
    for kind in ("cornell", "sponza"):
        pm, tm = [], []
        for rnd in range(args.rounds):
            a = run_child("frame:" + kind, args.parent_pkg, 240)
            b = run_child("frame:" + kind, "", 240)
            pm.append(med(a["ms"])); tm.append(med(b["ms"]))
            out.append(f"| {kind} | {rnd} | {med(a['ms']):.3f}; {min(a['ms']):.3f} .. {max(a['ms']):.3f} | {med(b['ms']):.3f}; {min(b['ms']):.3f} .. {max(b['ms']):.3f} |")
        spread, diff = max(pm) - min(pm), med(tm) - med(pm)
        ok = abs(diff) <= spread or diff < 0
        verdicts.append(f"* {kind}: parent {med(pm):.3f} ms (its rounds spread over {spread:.3f} ms), this {med(tm):.3f} ms, difference {diff:+.3f} ms: " +
                        ("inside the parent's own spread (or faster)" if ok else "OUTSIDE the parent's own spread"))
    out += [""] + verdicts + [""]
    rows = run_child("adaptive", "", 420)
    plain = med(rows[0]["ms"])
    out += ["## What the feature buys: Cornell, cap 64, min 8 / step 8 (reporting only)", "",
            "| call | wall ms (median; min .. max) | vs rtx_render | passes | pixel-samples | of 64 spp | chunks converged / at cap / all | RMSE vs 1 024 spp |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        ch = f"{r['converged']} / {r['at_max']} / {r['chunks']}" if "chunks" in r else "-"
        out.append(f"| {r['what']} | {med(r['ms']):.3f}; {min(r['ms']):.3f} .. {max(r['ms']):.3f} | {med(r['ms']) / plain:.3f} | {r['passes']} | {r['samples']} | {r['samples'] / (W * H * CAP):.3f} | {ch} | {r['rmse']:.5f} |")
    z = rows[1]
    out += ["", f"Per-pass cost (threshold 0 does rtx_render's work in {z['passes']} passes): {med(z['ms']) - plain:+.3f} ms over plain rtx_render, {(med(z['ms']) - plain) / max(z['passes'], 1):+.3f} ms per pass "
            "(criterion, list, read-back, and the launch tails of a frame cut into passes).", ""]
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    child() if args.child else main()

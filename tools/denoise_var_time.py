#!/usr/bin/env python3
"""What rtx_denoise_variance costs beside rtx_denoise, measured on the GPU with RTX_OPT_KERNEL_TIMING; writes a markdown report.

The scene and method of tools/denoise_maps_time.py: the Cornell box at 1920 x 1080 with a 256 x 256 texture bound as map_Kd and as normal map on its four non-emitting
materials, sampled with 16 spp by rtx_render_adaptive at threshold 0 (rtx_render's image, plus the second sum the variance-guided filter reads).  Per flags word 0 .. 3 and
per entry point: levels = 1 .. 5; rtx_denoise_result gives the guides and the filter as two hipEvent intervals, and the time of level i is filter_ms(levels = i + 1) -
filter_ms(levels = i).  Each measurement is a process of its own (--child); with --parent DIR (a built checkout of the parent commit) the parent's two entry points are
measured too, the two trees ALTERNATING round by round.
    python tools/denoise_var_time.py [--parent DIR] [--rounds 5] [--out profiles/denoise_var_time.md]"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS, SPP, REPS = 1920, 1080, 5, 16, 5
med = statistics.median


def child(root):
    """one process: per entry point and flags word the median over REPS calls of guides_ms and of filter_ms at levels 1 .. 5 -> one JSON line"""
    sys.path.insert(0, root)
    import numpy as np
    import __graft_entry__ as g
    rt = g.load_package()
    sc = rt.Scene.cornell()
    c = rt.Context(0)
    c.set_option(rt.OPT_KERNEL_TIMING, 1)
    c.upload(sc, W / H)
    rng = np.random.default_rng(1)
    c.set_mesh_uvs(0, rng.uniform(0.0, 4.0, (len(sc.meshes[0][1]), 2)).astype(np.float32))
    c.set_texture(0, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), False)
    for m in range(4):
        c.set_material_map(m, 0); c.set_material_map(m, 0, rt.MAP_NORMAL)
    c.commit()
    c.clear(W, H); c.render_adaptive(rt.Params(width=W, height=H, max_bounces=8, nee_samples=1, flags=0), SPP, SPP, SPP, 0.0)
    out = {}
    for variance in ((False, True) if hasattr(rt, "DenoiseVarParams") else (False,)):
        for fl in range(4):
            kw = dict(albedo=bool(fl & 1), mapped_normals=bool(fl & 2))
            if variance:
                kw["variance"] = True
            c.denoise(W, H, LEVELS, **kw)                               # warm-up: code objects, buffers
            guides, filt = [], []
            for lv in range(1, LEVELS + 1):
                rs = [c.denoise(W, H, lv, **kw) for _ in range(REPS)]
                filt.append(med(r.filter_ms for r in rs)); guides += [r.guides_ms for r in rs]
            out[("v" if variance else "d") + str(fl)] = dict(guides=med(guides), filter=filt)
    c.close()
    print("RESULT " + json.dumps(out))


def run(root):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"child failed ({r.returncode}): {r.stdout[-500:]} {r.stderr[-1500:]}")
    return json.loads(line[0][7:])


def spread(v):
    return f"{med(v):.4f} ({min(v):.4f} .. {max(v):.4f})"


def rows_of(runs, key):
    """the report's rows of one entry point and flags word: guides, the five levels, their sum -> list of value lists"""
    rows = [[r[key]["guides"] for r in runs]]
    for lv in range(LEVELS):
        rows.append([r[key]["filter"][lv] - (r[key]["filter"][lv - 1] if lv else 0.0) for r in runs])
    rows.append([r[key]["filter"][LEVELS - 1] for r in runs])
    return rows


LABELS = ["guides"] + [f"level {lv} (step {1 << lv})" for lv in range(LEVELS)] + [f"all {LEVELS} levels"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    new, old = [], []
    for rnd in range(args.rounds):
        order = [("new", ROOT)] + ([("old", args.parent)] if args.parent else [])
        for name, root in (order if rnd % 2 == 0 else order[::-1]):
            {"new": new, "old": old}[name].append(run(root))
            print(f"round {rnd} {name} done", flush=True)
    out = ["# rtx_denoise_variance beside rtx_denoise: time per level and flags word", "",
           f"One MI355X, Cornell box with a 256 x 256 map_Kd and normal map on its four non-emitting materials, {W} x {H}, {SPP} spp (rtx_render_adaptive, threshold 0);",
           f"RTX_OPT_KERNEL_TIMING (hipEvent intervals around the guides kernel and around the level kernels), RTX_OPT_DENOISE_LDS_STEP 4.  {args.rounds} rounds, every measurement a",
           f"process of its own, the trees alternating round by round; inside a process the median of {REPS} calls; below: the median over the rounds (min .. max over the rounds =",
           "the run-to-run spread), in ms.  Level i has step 1 << i.", ""]
    if old:
        for e, entry in (("d", "rtx_denoise"), ("v", "rtx_denoise_variance")):
            if not all(f"{e}0" in r for r in old):
                continue                                                # (a parent from before the variance-guided filter)
            out += [f"## {entry} against the parent commit", "",
                    "| | " + " | ".join(f"flags {f}: parent | flags {f}: this tree" for f in range(4)) + " |", "|---|" + "---|" * 8]
            cols = [rows_of(runs, f"{e}{f}") for f in range(4) for runs in (old, new)]
            for i, label in enumerate(LABELS):
                out.append(f"| {label} | " + " | ".join(spread(c[i]) for c in cols) + " |")
            out.append("")
    out += ["## rtx_denoise (d) and rtx_denoise_variance (v) on this tree", "", "| | " + " | ".join(f"d, flags {f} | v, flags {f}" for f in range(4)) + " |", "|---|" + "---|" * 8]
    cols = [rows_of(new, f"{e}{f}") for f in range(4) for e in "dv"]
    for i, label in enumerate(LABELS):
        out.append(f"| {label} | " + " | ".join(spread(c[i]) for c in cols) + " |")
    text = "\n".join(out) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""What rtx_denoise's map guides cost (RTX_DENOISE_ALBEDO = 1, RTX_DENOISE_MAPPED_NORMALS = 2), measured on the GPU with RTX_OPT_KERNEL_TIMING; writes a markdown report.

The Cornell box at 1920 x 1080, 16 spp, with a 256 x 256 texture bound as map_Kd and as normal map on its four non-emitting materials (so the guide kernel samples both).
Per flags word 0 .. 3: rtx_denoise with levels = 1 .. 5; rtx_denoise_result gives the guides and the filter as two hipEvent intervals, and the time of level i is
filter_ms(levels = i + 1) - filter_ms(levels = i), as in tools/denoise_time.py.  Each measurement is a process of its own (--child); with --parent DIR (a built checkout of the
parent commit) the parent's flags == 0 is measured too, the two trees ALTERNATING round by round, and the report states the difference with its run-to-run spread.
--lds-step 2 makes the step-4 level run direct (the alternative to the 72-KiB staged form of flag 2).
    python tools/denoise_maps_time.py [--parent DIR] [--rounds 5] [--out profiles/denoise_maps_time.md]"""
import argparse, json, os, statistics, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS, SPP, REPS = 1920, 1080, 5, 16, 5
med = statistics.median


def child(root, lds_step):
    """one process: per flags word the median over REPS calls of guides_ms and of filter_ms at levels 1 .. 5 -> one JSON line"""
    sys.path.insert(0, root)
    import numpy as np
    import __graft_entry__ as g
    rt = g.load_package()
    flags_list = (0, 1, 2, 3) if hasattr(rt, "DENOISE_ALBEDO") else (0,)
    sc = rt.Scene.cornell()
    c = rt.Context(0)
    c.set_option(rt.OPT_KERNEL_TIMING, 1)
    c.set_option(rt.OPT_DENOISE_LDS_STEP, lds_step)
    c.upload(sc, W / H)
    rng = np.random.default_rng(1)
    c.set_mesh_uvs(0, rng.uniform(0.0, 4.0, (len(sc.meshes[0][1]), 2)).astype(np.float32))
    c.set_texture(0, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), False)
    for m in range(4):
        c.set_material_map(m, 0); c.set_material_map(m, 0, rt.MAP_NORMAL)
    c.commit()
    c.clear(W, H); c.render(rt.Params(width=W, height=H, spp=SPP, max_bounces=8, nee_samples=1, flags=0))
    out = {}
    for fl in flags_list:
        kw = dict(albedo=bool(fl & 1), mapped_normals=bool(fl & 2)) if fl else {}
        c.denoise(W, H, LEVELS, **kw)                               # warm-up: code objects, buffers
        guides, filt = [], []
        for lv in range(1, LEVELS + 1):
            rs = [c.denoise(W, H, lv, **kw) for _ in range(REPS)]
            filt.append(med(r.filter_ms for r in rs)); guides += [r.guides_ms for r in rs]
        out[str(fl)] = dict(guides=med(guides), filter=filt)
    c.close()
    print("RESULT " + json.dumps(out))


def run(root, lds_step):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, "--lds-step", str(lds_step)], capture_output=True, text=True, timeout=600)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        raise SystemExit(f"child failed ({r.returncode}): {r.stdout[-500:]} {r.stderr[-1500:]}")
    return json.loads(line[0][7:])


def spread(v):
    return f"{med(v):.4f} ({min(v):.4f} .. {max(v):.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", default="")
    ap.add_argument("--lds-step", type=int, default=4)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.lds_step)
    new, old, new2 = [], [], []
    for rnd in range(args.rounds):
        order = [("new", ROOT, 4), ("new2", ROOT, 2)] + ([("old", args.parent, 4)] if args.parent else [])
        for name, root, lds in (order if rnd % 2 == 0 else order[::-1]):
            {"new": new, "old": old, "new2": new2}[name].append(run(root, lds))
    out = ["# rtx_denoise with map guides: time per level and flags word", "",
           f"One MI355X, Cornell box with a 256 x 256 map_Kd and normal map on its four non-emitting materials, {W} x {H}, {SPP} spp; RTX_OPT_KERNEL_TIMING (hipEvent intervals",
           f"around the guides kernel and around the level kernels).  {args.rounds} rounds, every measurement a process of its own, the trees and forms alternating round by round; inside a",
           f"process the median of {REPS} calls; below: the median over the rounds (min .. max over the rounds = the run-to-run spread).  Level i has step 1 << i.", ""]
    if old:
        out += ["## flags == 0 against the parent commit (expected difference: none — the same kernels are launched)", "", "| | parent ms | this tree ms |", "|---|---|---|"]
        out.append(f"| guides | {spread([r['0']['guides'] for r in old])} | {spread([r['0']['guides'] for r in new])} |")
        for lv in range(LEVELS):
            out.append(f"| filter, levels = {lv + 1} | {spread([r['0']['filter'][lv] for r in old])} | {spread([r['0']['filter'][lv] for r in new])} |")
        out.append("")

    def table(rows, title):
        t = [title, "", "| | flags 0 | flags 1 (albedo) | flags 2 (mapped normals) | flags 3 |", "|---|---|---|---|---|"]
        t.append("| guides | " + " | ".join(spread([r[str(f)]["guides"] for r in rows]) for f in range(4)) + " |")
        for lv in range(LEVELS):
            cells = []
            for f in range(4):
                cells.append(spread([r[str(f)]["filter"][lv] - (r[str(f)]["filter"][lv - 1] if lv else 0.0) for r in rows]))
            t.append(f"| level {lv} (step {1 << lv}) | " + " | ".join(cells) + " |")
        t.append(f"| all {LEVELS} levels | " + " | ".join(spread([r[str(f)]["filter"][LEVELS - 1] for r in rows]) for f in range(4)) + " |")
        t.append("| guides + levels | " + " | ".join(spread([r[str(f)]["guides"] + r[str(f)]["filter"][LEVELS - 1] for r in rows]) for f in range(4)) + " |")
        return t + [""]
    out += table(new, "## RTX_OPT_DENOISE_LDS_STEP 4 (default: steps 1, 2 and 4 staged; flags 2 and 3 stage 64 B per pixel, 72 KiB at step 4)")
    out += table(new2, "## RTX_OPT_DENOISE_LDS_STEP 2 (step 4 direct: the alternative to the 72-KiB form)")
    text = "\n".join(out)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(text)


if __name__ == "__main__":
    main()

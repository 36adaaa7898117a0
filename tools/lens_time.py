#!/usr/bin/env python3
"""What the thin-lens camera costs (profiles/lens_time.md): python tools/lens_time.py <plain|lens> [frames=4] [figures=3]
plain: the headline frame (Cornell box, 1080p, 64 spp, 8 bounces, Lambert) with no lens call at all — runs from a checkout of the parent commit too, for the alternating comparison
lens:  the headline frame and the atrium (262 k triangles, 1080p, 16 spp) with the lens off, on, off, on in ONE context each (the headline also with the lens off and
       RTX_OPT_SHARED_PRIMARY 0: what the shared primary hit alone is worth): aperture radius = 1 % of the scene's largest extent,
       focus = rtx_focus_distance_at the image centre; per state ms per frame (wall time per rtx_render, `figures` figures of `frames` frames), rays, launches per kernel class"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); os.chdir(ROOT)
import numpy as np
import __graft_entry__ as g
rt = g.load_package()
mode = sys.argv[1] if len(sys.argv) > 1 else "plain"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
figures = int(sys.argv[3]) if len(sys.argv) > 3 else 3
W, H = 1920, 1080


def figures_of(c, p):
    out = []
    for _ in range(figures):
        t0 = time.perf_counter()
        for _ in range(frames):
            c.render(p)                      # synchronous on the context's own stream
        out.append((time.perf_counter() - t0) * 1e3 / frames)
    return out


def workload(name):
    sc = rt.Scene.cornell() if name == "headline" else rt.Scene.sponza_class()
    c = rt.Context(0)
    c.upload(sc, W / H)
    p = rt.Params(width=W, height=H, spp=64 if name == "headline" else 16, max_bounces=8, nee_samples=1, rr_start=3, sample_base=1, flags=1)
    c.clear(W, H); c.render(p); c.render(p)                      # warm-up
    return sc, c, p


if mode == "plain":
    sc, c, p = workload("headline")
    ms = figures_of(c, p)
    st = c.stats()
    print(f"headline, no lens call: {' '.join(f'{m:.3f}' for m in ms)} ms per frame; rays {st.rays}", flush=True)
    c.close()
else:
    for name in ("headline", "atrium"):
        sc, c, p = workload(name)
        lo, hi = sc.bounds()
        radius = 0.01 * float((hi - lo).max())
        focus = float(c.focus_distance_at(W, H, W // 2, H // 2))
        print(f"{name}: aperture radius {radius:.4g}, focus {focus:.4g} (autofocus at the image centre)", flush=True)
        states = ("off", "on", "off", "on") + (("off, RTX_OPT_SHARED_PRIMARY 0",) * 2 if name == "headline" else ())      # the last: per-sample primary rays WITH packet culling
        for state in states:
            c.set_lens(radius if state == "on" else 0.0, focus)
            c.set_option(rt.OPT_SHARED_PRIMARY, 0 if "SHARED" in state else 1)
            c.render(p)                                              # the state's first frame is not timed
            ms = figures_of(c, p)
            st = c.stats()
            ln = {rt.KERNEL_NAMES[k]: int(st.kernel_launches[k]) for k in range(rt.K_COUNT) if st.kernel_launches[k]}
            print(f"  lens {state}: {' '.join(f'{m:.3f}' for m in ms)} ms per frame; rays {st.rays_primary} / {st.rays_extension} / {st.rays_shadow} = {st.rays / (min(ms) * 1e3):.0f} Mrays/s; launches {ln}", flush=True)
        c.close()

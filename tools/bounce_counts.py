#!/usr/bin/env python3
"""Tooling: rays per bounce of a workload (queue lengths entering each bounce), from runs with max_bounces = 1..8.
usage: python tools/bounce_counts.py [sponza|bistro|cornell]     (cornell: the headline frame of bench.py — 64 spp, Lambert-only, the fused tiny-scene path)"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
kind = sys.argv[1] if len(sys.argv) > 1 else "sponza"
sc = {"sponza": rt.Scene.sponza_class, "bistro": rt.Scene.bistro_class, "cornell": rt.Scene.cornell}[kind]()
W, H = 1920, 1080
spp, flags = {"sponza": (4, 1), "bistro": (4, 4), "cornell": (64, 1)}[kind]
c = rt.Context(0); c.upload(sc, W / H)
prev_ext = prev_sh = 0
for mb in range(1, 9):
    p = rt.Params(width=W, height=H, spp=spp, max_bounces=mb, nee_samples=1, flags=flags)
    c.clear(W, H); c.render(p); st = c.stats()
    n = st.rays_primary if mb == 1 else st.rays_extension - prev_ext
    print(f"{kind} bounce {mb - 1}: {n} rays, {n / st.rays_primary:.3f} of the primary rays traced, shadow rays {(st.rays_shadow - prev_sh) / st.rays_primary:.3f}")
    prev_ext, prev_sh = st.rays_extension, st.rays_shadow
c.close()

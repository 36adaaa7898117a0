#!/usr/bin/env python3
"""Tooling: what an emission map costs.  The 262 k-triangle atrium at 1080p, 16 spp, 8 bounces, default flags (GGX), with procedural per-corner UVs (world x + z, y of the
corner, one repeat per unit) in four states of ONE context, alternating and warm: no emission map; one 1024 x 1024 noise texture as RTX_MAP_KE of every emissive material
(k_shade<.., EMI> runs: a texel fetch at every triangle-light NEE sample and at every emissive hit, the light weights follow the texels); the same size of map with
all-255 texels (the same kernel and fetches, the image is the unmapped one); no emission map again.  Per state the time of the commit that entered it, the wall time of a
frame with RTX_OPT_KERNEL_TIMING off, and the per-kernel-class times (HIP events) with it on.  The wave caps of the EMI forms are build-time constants: run the tool once
per library (RTX_LIB_PATH=librtx_hip_<variant>.so, built with `make VARIANT=<variant> VARFLAGS=-DRTX_SHADE_WAVES_EMI=N`) for an A/B against their neighbours.
usage: python tools/emimap_time.py [frames] [rounds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
W, H = 1920, 1080
print("library:", rt.LIB_PATH, flush=True)
sc = rt.Scene.sponza_class()
p = rt.Params(width=W, height=H, spp=16, max_bounces=8, nee_samples=1, rr_start=3, sample_base=1, flags=0)
c = rt.Context(0)
c.upload(sc, W / H)
emitters = [m for m in range(len(sc.materials)) if (np.asarray(sc.materials[m][8:11]) > 0).any()]


def wall(n):
    c.clear(W, H)
    t0 = time.perf_counter()
    for f in range(n):
        c.render(p.copy(frame_seed=1 + f))
    return (time.perf_counter() - t0) * 1e3 / n


def commit():
    t0 = time.perf_counter()
    c.commit()
    return (time.perf_counter() - t0) * 1e3


def run(tag, commit_ms=None):
    c.set_option(rt.OPT_KERNEL_TIMING, 0)
    wall(1)
    ms = [wall(frames) for _ in range(rounds)]
    c.set_option(rt.OPT_KERNEL_TIMING, 1)
    rows = []
    for rep in range(frames + 1):
        c.clear(W, H); c.render(p.copy(frame_seed=1))
        s = c.stats()
        if rep:
            rows.append((s.kernel_ms[rt.K_TRACE], s.kernel_ms[rt.K_SHADE], s.kernel_ms[rt.K_SHADOW]))
    a = np.array(rows)
    s = c.stats()
    print(f"{tag}: " + (f"commit {commit_ms:.1f} ms; " if commit_ms is not None else "") + "frame " + " ".join(f"{t:.2f}" for t in ms) + f" ms (median {np.median(ms):.2f}); "
          f"k_trace_closest {np.median(a[:, 0]):.2f}, k_shade {np.median(a[:, 1]):.2f} (min {a[:, 1].min():.2f}, max {a[:, 1].max():.2f}), k_trace_shadow {np.median(a[:, 2]):.2f} ms; "
          f"shaded items {s.kernel_items[rt.K_SHADE]}, shadow rays {s.rays_shadow}, lights {s.lights}, bvh_refits {s.bvh_refits}", flush=True)
    return c.read_accum()


plain = run("no emission map")
for mesh, (v, i, m) in enumerate(sc.meshes):
    pos = np.asarray(v, np.float32)[np.asarray(i, np.int64), :3]
    c.set_mesh_uvs(mesh, np.stack([pos[:, 0] + pos[:, 2], pos[:, 1]], 1))
rng = np.random.default_rng(1)
noise = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
c.set_texture(0, noise, False)
for m in emitters:
    c.set_material_map(m, 0, rt.MAP_KE)
noisy = run(f"1024^2 noise map on {len(emitters)} emissive materials", commit())
c.set_texture(0, np.full((1024, 1024, 4), 255, np.uint8), False)
white = run("1024^2 all-255 map", commit())
for m in emitters:
    c.set_material_map(m, -1, rt.MAP_KE)
again = run("no emission map again", commit())
print("images: unmapped == all-255 map:", bool(np.array_equal(plain, white)), "; == unmapped again:", bool(np.array_equal(plain, again)), "; the noise map differs:", bool(not np.array_equal(plain, noisy)))
c.close()

#!/usr/bin/env python3
"""Tooling: what specular, roughness and metalness maps cost.  The 262 k-triangle atrium at 1080p, 16 spp, 8 bounces, default flags (GGX), with procedural per-corner UVs
(world x + z, y of the corner, one repeat per unit) in four states of ONE context, alternating and warm: no specular map; one 1024 x 1024 noise texture in all three slots
(RTX_MAP_KS / PR / PM) of every non-emissive material plus a 17-row energy table; the same size of map with all-255 texels and no table (k_shade<.., SPC> runs and reads
every tap, the image is the unmapped one); no specular map again.  Per state the wall time of a frame with RTX_OPT_KERNEL_TIMING off, and the per-kernel-class times (HIP
events) with it on.  The wave cap of the SPC forms is a build-time constant: run the tool once per library (RTX_LIB_PATH=librtx_hip_<variant>.so, built with
`make VARIANT=<variant> VARFLAGS=-DRTX_SHADE_WAVES_SPC=N`) for the A/B against its neighbours.
usage: python tools/specmap_time.py [frames] [rounds]"""
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
mapped = [m for m in range(len(sc.materials)) if not (np.asarray(sc.materials[m][8:11]) > 0).any()]
SLOTS = (rt.MAP_KS, rt.MAP_PR, rt.MAP_PM)


def wall(n):
    c.clear(W, H)
    t0 = time.perf_counter()
    for f in range(n):
        c.render(p.copy(frame_seed=1 + f))
    return (time.perf_counter() - t0) * 1e3 / n


def run(tag):
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
    print(f"{tag}: frame " + " ".join(f"{t:.2f}" for t in ms) + f" ms (median {np.median(ms):.2f}); k_trace_closest {np.median(a[:, 0]):.2f}, k_shade {np.median(a[:, 1]):.2f} "
          f"(min {a[:, 1].min():.2f}, max {a[:, 1].max():.2f}), k_trace_shadow {np.median(a[:, 2]):.2f} ms; shaded items {c.stats().kernel_items[rt.K_SHADE]}", flush=True)
    return c.read_accum()


def bind(tex):
    for m in mapped:
        for slot in SLOTS:
            c.set_material_map(m, tex, slot)


plain = run("no specular map")
for mesh, (v, i, m) in enumerate(sc.meshes):
    pos = np.asarray(v, np.float32)[np.asarray(i, np.int64), :3]
    c.set_mesh_uvs(mesh, np.stack([pos[:, 0] + pos[:, 2], pos[:, 1]], 1))
rng = np.random.default_rng(1)
noise = rng.integers(0, 256, (1024, 1024, 4), dtype=np.uint8)
c.set_texture(0, noise, False)
bind(0)
c.set_ess_table(rt.ess_table_rows(17))
c.commit()
noisy = run(f"1024^2 noise map in all three slots of {len(mapped)} materials + a 17-row table")
c.set_texture(0, np.full((1024, 1024, 4), 255, np.uint8), False); c.set_ess_table(None); c.commit()
white = run("1024^2 all-255 map in all three slots, no table")
bind(-1)
c.commit()
again = run("no specular map again")
print("images: unmapped == all-255 map:", bool(np.array_equal(plain, white)), "; == unmapped again:", bool(np.array_equal(plain, again)), "; the noise map differs:", bool(not np.array_equal(plain, noisy)))
c.close()

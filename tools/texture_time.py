#!/usr/bin/env python3
"""Tooling: what diffuse texture maps cost.  The 262 k-triangle atrium at 1080p, 16 spp, 8 bounces with procedural per-corner UVs (world x + z, y of the corner, one repeat per
unit) and one 1024 x 1024 noise texture mapped to every non-emissive material, against the same context unmapped: frame time and per-kernel-class time (HIP events).
usage: python tools/texture_time.py [frames]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
sc = rt.Scene.sponza_class()
W, H = 1920, 1080
c = rt.Context(0)
c.set_option(rt.OPT_KERNEL_TIMING, 1)
c.upload(sc, W / H)
p = rt.Params(width=W, height=H, spp=16, max_bounces=8, nee_samples=1, flags=0)


def run(tag):
    rows = []
    for rep in range(frames + 1):
        c.clear(W, H); c.render(p)
        st = c.stats()
        if rep:
            rows.append((st.render_ms, st.kernel_ms[rt.K_TRACE], st.kernel_ms[rt.K_SHADE], st.kernel_ms[rt.K_SHADOW]))
    a = np.array(rows)
    print(f"{tag}: frame {np.median(a[:, 0]):.2f} ms (min {a[:, 0].min():.2f}, max {a[:, 0].max():.2f}); k_trace_closest {np.median(a[:, 1]):.2f}, k_shade {np.median(a[:, 2]):.2f} "
          f"(min {a[:, 2].min():.2f}, max {a[:, 2].max():.2f}), k_trace_shadow {np.median(a[:, 3]):.2f}; shaded items {c.stats().kernel_items[rt.K_SHADE]}", flush=True)
    return c.read_accum()


plain = run("unmapped")
for mesh, (v, i, m) in enumerate(sc.meshes):
    pos = np.asarray(v, np.float32)[np.asarray(i, np.int64), :3]
    c.set_mesh_uvs(mesh, np.stack([pos[:, 0] + pos[:, 2], pos[:, 1]], 1))
c.set_texture(0, np.random.default_rng(1).integers(0, 256, (1024, 1024, 4), dtype=np.uint8), True)
mapped = [k for k in range(len(sc.materials)) if not sc.materials[k][8:11].any()]
for k in mapped:
    c.set_material_map(k, 0)
c.commit()
tex = run(f"1024^2 map on {len(mapped)} materials")
for k in mapped:
    c.set_material_map(k, -1)
c.commit()
again = run("unmapped again")
print("images: unmapped == unmapped again:", bool(np.array_equal(plain, again)), "; mapped differs:", bool(not np.array_equal(plain, tex)))
c.close()

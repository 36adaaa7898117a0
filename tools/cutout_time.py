#!/usr/bin/env python3
"""Tooling: what alpha cut-outs cost.  Two modes, both at 1080p on one GPU, RTX_OPT_KERNEL_TIMING off for frame times and on for the per-kernel-class times (HIP events).
  plain  headline (Cornell box, 64 spp, Lambert), C3 (262 k-triangle atrium, 16 spp) and C5 (3.8 M-triangle street, 16 spp, transmission) WITHOUT cut-outs: wall ms per
         frame.  Uses nothing this feature added, so it runs unchanged from a checkout of the parent: run it alternately from both trees on the same box for the A/B.
  cost   the atrium with procedural per-corner UVs in three states of ONE context: unmapped; an all-255 256 x 256 opacity map on every non-emissive material (the CUT
         kernels run, no candidate is rejected, the image is bit-identical: the pure cost of the instantiations); the same map with 50 % of its 8 x 8 blocks at alpha 0
         (rays pass through half of every surface: longer rays, more of them).  Frame ms, k_trace_closest / k_shade / k_trace_shadow ms, rays per second, and node steps /
         triangle tests per ray from the traversal's own counters (RTX_OPT_TRACE_COUNTERS, a second context: the counters select the generic instantiations).
usage: python tools/cutout_time.py plain|cost [frames] [rounds]"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
mode = sys.argv[1] if len(sys.argv) > 1 else "cost"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 4
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
W, H = 1920, 1080
print("library:", rt.LIB_PATH, flush=True)


def wall(c, p, n):
    c.clear(W, H)
    t0 = time.perf_counter()
    for f in range(n):
        c.render(p.copy(frame_seed=1 + f))
    return (time.perf_counter() - t0) * 1e3 / n


if mode == "plain":
    work = [("headline", rt.Scene.cornell, dict(spp=64, flags=rt.FLAG_LAMBERT_ONLY)), ("C3", rt.Scene.sponza_class, dict(spp=16, flags=rt.FLAG_LAMBERT_ONLY)),
            ("C5", rt.Scene.bistro_class, dict(spp=16, flags=rt.FLAG_TRANSMISSION))]
    for name, ctor, kw in work:
        sc = ctor()
        c = rt.Context(0)
        c.upload(sc, W / H)
        p = rt.Params(width=W, height=H, max_bounces=8, nee_samples=1, rr_start=3, sample_base=1, **kw)
        wall(c, p, 1)                                            # warm-up (allocations)
        ms = [wall(c, p, frames) for _ in range(rounds)]
        st = c.stats()
        print(f"{name}: " + " ".join(f"{t:.3f}" for t in ms) + f" ms/frame (min {min(ms):.3f}, median {np.median(ms):.3f}); rays {st.rays_primary + st.rays_extension + st.rays_shadow}", flush=True)
        c.close()
    sys.exit(0)

sc = rt.Scene.sponza_class()
p = rt.Params(width=W, height=H, spp=16, max_bounces=8, nee_samples=1, rr_start=3, sample_base=1, flags=0)
c = rt.Context(0)
c.upload(sc, W / H)
k = rt.Context(0)                                               # the counting context
k.set_option(rt.OPT_TRACE_COUNTERS, 1)
k.upload(sc, W / H)
mapped = [m for m in range(len(sc.materials)) if not (np.asarray(sc.materials[m][8:11]) > 0).any()]


def run(tag):
    c.set_option(rt.OPT_KERNEL_TIMING, 0)
    wall(c, p, 1)
    ms = [wall(c, p, frames) for _ in range(rounds)]
    st = c.stats()
    rays = st.rays_primary + st.rays_extension + st.rays_shadow
    c.set_option(rt.OPT_KERNEL_TIMING, 1)
    rows = []
    for rep in range(frames + 1):
        c.clear(W, H); c.render(p.copy(frame_seed=1))
        s = c.stats()
        if rep:
            rows.append((s.kernel_ms[rt.K_TRACE], s.kernel_ms[rt.K_SHADE], s.kernel_ms[rt.K_SHADOW]))
    a = np.median(np.array(rows), 0)
    img = c.read_accum()
    k.clear(W, H); k.trace_counters(); k.render(p.copy(frame_seed=1))
    ks = k.stats(); n = k.trace_counters()
    nc, ns = ks.rays_primary + ks.rays_extension, max(ks.rays_shadow, 1)
    print(f"{tag}: frame " + " ".join(f"{t:.2f}" for t in ms) + f" ms (median {np.median(ms):.2f}), {rays / np.median(ms) / 1e3:.1f} Mrays/s; k_trace_closest {a[0]:.2f}, k_shade {a[1]:.2f}, "
          f"k_trace_shadow {a[2]:.2f} ms; rays primary {st.rays_primary} extension {st.rays_extension} shadow {st.rays_shadow}; per closest-hit ray {n[0] / nc:.1f} node steps, "
          f"{n[1] / nc:.1f} triangle tests; per any-hit ray {n[2] / ns:.1f}, {n[3] / ns:.1f}", flush=True)
    return img


def bind(ctx, tex):
    for mesh, (v, i, m) in enumerate(sc.meshes):
        pos = np.asarray(v, np.float32)[np.asarray(i, np.int64), :3]
        ctx.set_mesh_uvs(mesh, np.stack([pos[:, 0] + pos[:, 2], pos[:, 1]], 1))
    ctx.set_texture(0, tex, False)
    for m in mapped:
        ctx.set_material_map(m, 0 if tex is not None else -1, rt.MAP_OPACITY)
    ctx.commit()


plain = run("unmapped")
full = np.full((256, 256, 4), 255, np.uint8)
for ctx in (c, k):
    bind(ctx, full)
opaque = run(f"all-255 256^2 opacity map on {len(mapped)} materials")
half = full.copy()
half[..., 3] = np.repeat(np.repeat(np.random.default_rng(1).integers(0, 2, (32, 32), dtype=np.uint8) * 255, 8, 0), 8, 1)
for ctx in (c, k):
    ctx.set_texture(0, half, False); ctx.commit()
holes = run("50 % of the 8 x 8 blocks at alpha 0")
for ctx in (c, k):
    for m in mapped:
        ctx.set_material_map(m, -1, rt.MAP_OPACITY)
    ctx.commit()
again = run("unmapped again")
print("images: unmapped == all-255 map:", bool(np.array_equal(plain, opaque)), "; == unmapped again:", bool(np.array_equal(plain, again)), "; the holes differ:", bool(not np.array_equal(plain, holes)))
k.close(); c.close()

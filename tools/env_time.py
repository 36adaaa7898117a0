#!/usr/bin/env python3
"""Tooling: what environment lighting costs.  The 262 k-triangle atrium at 1080p, 16 spp, 8 bounces, RTX_OPT_KERNEL_TIMING on, in three states of ONE context: as shipped
(lit by its emissive sky quad), with a 512 x 512 environment beside the quad, and with the quad dark and the environment alone: frame time, per-kernel-class time (HIP
events) and rays per state.  The quad is part of the atrium's one mesh, so "without the quad" means its material's Ke set to 0 (rtx_set_materials), not a hidden instance.
The marginal CDF's place (LDS or global memory) is a compile-time choice: build the other form with `make VARIANT=envg VARFLAGS=-DRTX_ENV_MARG_GLOBAL` and run this tool
alternately with RTX_LIB_PATH pointing at librtx_hip_envg.so.
usage: python tools/env_time.py [frames] [env states only: 0 | 1]"""
import math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
frames = int(sys.argv[1]) if len(sys.argv) > 1 else 4
env_only = len(sys.argv) > 2 and sys.argv[2] == "1"
sc = rt.Scene.sponza_class()
W, H = 1920, 1080
c = rt.Context(0)
c.set_option(rt.OPT_KERNEL_TIMING, 1)
c.upload(sc, W / H)
p = rt.Params(width=W, height=H, spp=16, max_bounces=8, nee_samples=1, flags=0)


def sky(n):
    """a procedural outdoor sky as a lat-long image (2 n x n): horizon-to-zenith gradient, a dim ground, a 3-degree sun of 2000 x the sky 50 degrees up"""
    t = (np.arange(n) + 0.5) / n * math.pi
    ph = (np.arange(2 * n) + 0.5) / (2 * n) * 2.0 * math.pi
    T, P = np.meshgrid(t, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.sin(P), np.cos(T), -np.sin(T) * np.cos(P)], -1)
    up = np.clip(d[..., 1], 0.0, 1.0)
    img = np.where(d[..., 1:2] >= 0, (1.0 - up[..., None]) * np.array([0.9, 0.95, 1.0]) + up[..., None] * np.array([0.25, 0.45, 1.0]), np.array([0.12, 0.11, 0.1]))
    s = np.array([math.cos(math.radians(50)) * 0.6, math.sin(math.radians(50)), math.cos(math.radians(50)) * 0.8])
    img[(d @ s) > math.cos(math.radians(1.5))] = (2000.0, 1900.0, 1700.0)
    return img.astype(np.float32)


def run(tag):
    rows = []
    for rep in range(frames + 1):
        c.clear(W, H); c.render(p)
        st = c.stats()
        if rep:
            rows.append((st.render_ms, st.kernel_ms[rt.K_TRACE], st.kernel_ms[rt.K_SHADE], st.kernel_ms[rt.K_SHADOW]))
    a = np.array(rows)
    st = c.stats()
    print(f"{tag}: frame {np.median(a[:, 0]):.2f} ms (min {a[:, 0].min():.2f}, max {a[:, 0].max():.2f}); k_trace_closest {np.median(a[:, 1]):.2f}, k_shade {np.median(a[:, 2]):.2f} "
          f"(min {a[:, 2].min():.2f}, max {a[:, 2].max():.2f}), k_trace_shadow {np.median(a[:, 3]):.2f} (min {a[:, 3].min():.2f}, max {a[:, 3].max():.2f}); "
          f"rays primary {st.rays_primary} extension {st.rays_extension} shadow {st.rays_shadow}; shaded items {st.kernel_items[rt.K_SHADE]}", flush=True)
    return c.read_accum()


print("library:", rt.LIB_PATH, flush=True)
plain = None if env_only else run("as shipped")
env = rt.latlong_to_octahedral(sky(1024), 512)
c.set_environment(env); c.commit()
both = run("512^2 environment beside the sky quad")
mats = np.array(sc.materials, np.float32, copy=True)
mats[:, 8:11] = 0.0
c.set_materials(mats); c.set_environment(env); c.commit()
alone = run("environment alone (the quad's Ke = 0)")
if not env_only:
    c.set_materials(sc.materials); c.set_environment(None); c.commit()
    again = run("as shipped again")
    print("images: as shipped == as shipped again:", bool(np.array_equal(plain, again)), "; with the environment differs:", bool(not np.array_equal(plain, both)))
c.close()

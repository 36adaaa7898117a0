#!/usr/bin/env python3
"""Tooling: what a maps-only commit costs on the host.  The 262 k-triangle atrium, resident; the Kd slot of one material that triangles use is toggled between two 256 x 256
textures and every rtx_commit_scene is timed with a host clock (the commit ends in a stream synchronise: finalise_scene).  Such a commit uploads tables and refits nothing.
RTX_LIB_PATH picks the library, so two builds can be compared by running this once per build, alternating.
usage: python tools/mapslots_commit_time.py [commits]     prints one JSON line: median, min, max in ms"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch  # noqa
import __graft_entry__ as graft
rt = graft.load_package()
commits = int(sys.argv[1]) if len(sys.argv) > 1 else 40
sc = rt.Scene.sponza_class()
c = rt.Context(0)
c.upload(sc, 16 / 9)
rng = np.random.default_rng(1)
for t in range(2):
    c.set_texture(t, rng.integers(0, 256, (256, 256, 4), dtype=np.uint8), True)
mat = int(np.bincount(np.asarray(sc.meshes[0][2])[0::3]).argmax())      # the material most triangles use
c.set_material_map(mat, 1); c.commit()
refits, tree = c.stats().bvh_refits, c.tree_hash()
ms = []
for k in range(commits + 4):                                  # (the first four warm up: the first one allocates the tables)
    c.set_material_map(mat, k & 1)
    t0 = time.perf_counter()
    c.commit()
    ms.append((time.perf_counter() - t0) * 1e3)
assert (c.stats().bvh_refits, c.tree_hash()) == (refits, tree)      # tables only: the tree was neither rebuilt nor refitted
p = rt.Params(width=64, height=36)
ids = c.albedo(c.trace_closest(c.primary_rays(p)))[:, 3].copy().view(np.uint32)
mapped_hits = int(((ids == 0) | (ids == 1)).sum())                   # > 0: the map is ACTIVE, camera rays hit triangles whose Kd comes from it
a = np.array(ms[4:])
print(json.dumps(dict(lib=os.path.basename(os.path.dirname(rt.LIB_PATH)) + "/" + os.path.basename(rt.LIB_PATH), triangles=int(c.stats().triangles), mapped_hits=mapped_hits, commits=commits,
                      median_ms=round(float(np.median(a)), 4), min_ms=round(float(a.min()), 4), max_ms=round(float(a.max()), 4))), flush=True)
c.close()

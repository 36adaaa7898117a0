"""SHA-256 of the scene cache the host build writes, for a matrix of scenes and builder options (no GPU needed): python tools/host_build_hashes.py
One `name hash size anyhit_order` line per row.  A change that must leave the host build alone is checked by running this on both builds (RTX_LIB_PATH picks the library)
and comparing the two outputs; the hashes depend on the host compiler's libm, so they are compared between builds on one machine and never kept as expectations."""
import hashlib
import os
import sys
import tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402
rt = g.load_package()
GOLDEN = os.path.join(ROOT, "tests", "golden")
DEFAULTS = {"ploc": 0, "split": 0.0, "sweep": 0, "slot_assign": 0, "threads": 0, "leaf_stop": 1, "reinsert": 2}      # csrc/rtx_bvh_host.hpp: BvhBuildOptions


def hard100k():
    return rt.Scene.sponza_class(target_tris=100000, hard=True)


ROWS = [
    ("cornell", rt.Scene.cornell, {}),
    ("garage+monke", lambda: rt.Scene.from_obj([os.path.join(GOLDEN, "garage.obj"), os.path.join(GOLDEN, "monke.obj")], GOLDEN + "/"), {}),
    ("sponza20k", lambda: rt.Scene.sponza_class(target_tris=20000), {}),
    ("sponza100k_hard", hard100k, {}),
    ("bistro70k", lambda: rt.Scene.bistro_class(target_tris=70000), {}),
    ("sponza262k", rt.Scene.sponza_class, {}),
    ("sponza100k_hard:ploc=16", hard100k, {"ploc": 16}),
    ("sponza100k_hard:split=1e-5", hard100k, {"split": 1e-5}),
    ("sponza100k_hard:sweep=8,slot_assign=1", hard100k, {"sweep": 8, "slot_assign": 1}),
    ("sponza100k_hard:threads=1", hard100k, {"threads": 1}),
    ("sponza100k_hard:leaf_stop=2,reinsert=0", hard100k, {"leaf_stop": 2, "reinsert": 0}),
]

with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "scene.rtxscn")
    for name, make, opts in ROWS:
        for k, v in {**DEFAULTS, **opts}.items():
            rt.bvh_option(k, v)
        sc = make()
        sc.save(path)
        data = open(path, "rb").read()
        print(name, hashlib.sha256(data).hexdigest(), len(data), sc.anyhit_order(), flush=True)

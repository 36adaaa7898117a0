"""Wall time of vertex-changing commits (rtx_update_mesh_vertices + rtx_commit_scene) against the routes a caller had before: the scene re-added and re-committed in a fresh
context (host builder and RTX_OPT_GPU_BUILD; measured with --parent-pkg on the parent commit's built package directory, in a child process — one process holds one library), and against the
transform-only partial refit.  Then 30 steps of a growing deformation of the atrium: commit + frame time refitting only vs RTX_OPT_DEFORM_REBUILD 1, with the tree cost.
    python tools/deform_time.py [--parent-pkg DIR/royaltracer-dx_amd] [--out profiles/deform_time.md] [--no-street]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--parent-pkg", default="", help="the parent commit's royaltracer-dx_amd directory with its librtx_hip.so built")
ap.add_argument("--out", default="")
ap.add_argument("--no-street", action="store_true")
ap.add_argument("--fresh-only", default="", help="(child process) case name: print the fresh-context times as JSON and exit")
args = ap.parse_args()

import __graft_entry__ as g
if args.fresh_only and args.parent_pkg:
    g.PKG_DIR = os.path.abspath(args.parent_pkg)            # (child process: the parent commit's package and library)
rt = g.load_package()
GOLD = os.path.join(ROOT, "tests", "golden")


class Arrays:
    def __init__(self, big, small=None):
        self.materials = np.asarray(big.materials, np.float32); self.meshes = list(big.meshes); self.instances = list(big.instances); self._big = big
        if small is not None:
            nm = len(big.materials); base = sum(len(m) for _, _, m in big.meshes)
            self.materials = np.concatenate([self.materials, np.asarray(small.materials, np.float32)])
            for v, i, m in small.meshes:
                v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)
                self.meshes.append((v, i, np.asarray(m, np.uint32) + np.uint32(nm))); base += len(m)
            place = np.eye(4, dtype=np.float32); place[0, 0] = place[1, 1] = place[2, 2] = 0.25; place[3, 1] = 0.3
            self.instances += [(len(big.meshes) + mesh, place.reshape(16)) for mesh, _ in small.instances]
    def view_proj(self, aspect): return self._big.view_proj(aspect)


def wave(v, amp, phase):
    """a travelling sine in y over x: cheap, and every vertex moves"""
    w = np.array(v, np.float32, copy=True); w[:, 1] += (amp * np.sin(8.0 * w[:, 0] + phase)).astype(np.float32)
    return w


def cases():
    monke = rt.Scene.from_obj([os.path.join(GOLD, "monke.obj")], GOLD + "/")
    atrium = rt.Scene.sponza_class()
    yield "monke in the 262 k atrium", Arrays(atrium, monke), "last"
    yield "the whole 262 k atrium", Arrays(atrium), "all"
    if not args.no_street:
        yield "the whole 3.8 M street", Arrays(rt.Scene.bistro_class()), "all"


def fresh_times(sc):
    """the scene handed over and committed in a new context: the only route to new vertices before rtx_update_mesh_vertices"""
    out = {}
    for tag, gb in (("host builder", 0), ("RTX_OPT_GPU_BUILD", 1)):
        ts = []
        for k in range(2):
            c = rt.Context(0); c.set_option(rt.OPT_GPU_BUILD, gb); t0 = time.time(); c.upload(sc, 16 / 9); ts.append((time.time() - t0) * 1e3); c.close()
        out[tag] = min(ts)
    return out


if args.fresh_only:
    for name, sc, _ in cases():
        if name == args.fresh_only:
            print("FRESH " + json.dumps(fresh_times(sc)))
    sys.exit(0)

lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)

say("# Vertex-changing commits (tools/deform_time.py): wall time of rtx_update_mesh_vertices + rtx_commit_scene")
say()
say("env: " + " ".join(f"{k}={os.environ[k]}" for k in sorted(os.environ) if k.startswith(("HIP_", "HSA_", "GPU_", "ROCR_", "OMP_NUM"))) + " | fresh-context rows measured on " + ("the parent commit's library" if args.parent_pkg else "THIS library (no --parent-pkg)"))
say()
say("All times in ms, wall clock around the call (a commit ends with a stream synchronise).  `update` = rtx_update_mesh_vertices (validation + host copy), `commit` = the commit that follows;")
say("first = the first vertex-changing commit of the context (a host-built scene fills the device mesh pool and takes its cost baseline there), then the median of 5 more.")
say()
say("```")
med = lambda a: float(np.median(a))
for name, sc, which in cases():
    meshes = [len(sc.meshes) - 1] if which == "last" else list(range(len(sc.meshes)))
    ntri = sum(len(sc.meshes[m][1]) // 3 for m, _ in sc.instances)
    say(f"== {name}: {ntri} triangles, deforming {sum(len(sc.meshes[m][1]) // 3 for m in meshes)} ==")
    if args.parent_pkg:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fresh-only", name, "--parent-pkg", args.parent_pkg] + (["--no-street"] if args.no_street else []), capture_output=True, text=True, timeout=900)
        got = [l for l in p.stdout.splitlines() if l.startswith("FRESH ")]
        if p.returncode != 0 or not got:
            say("fresh context on the parent's library: FAILED " + p.stderr[-300:]); fr = {}
        else:
            fr = json.loads(got[0][6:])
    else:
        fr = fresh_times(sc)
    for tag, ms in fr.items():
        say(f"fresh context, re-add + commit, {tag:18s}: {ms:9.2f}")
    for tag, opts in (("host-built tree", []), ("GPU-built tree", [(rt.OPT_GPU_BUILD, 1)]), ("host refit (GPU_REFIT 0)", [(rt.OPT_GPU_REFIT, 0)])):
        if tag.startswith("host refit") and ntri > 1000000:
            continue
        c = rt.Context(0)
        for o, v in opts:
            c.set_option(o, v)
        c.upload(sc, 16 / 9)
        inst = len(sc.instances) - 1
        tr = []
        for k in range(6):                                       # the transform-only partial refit of the same instance(s): the yardstick
            m = np.array(sc.instances[inst][1], np.float32, copy=True).reshape(4, 4); m[3, 1] += 0.01 * (k + 1)
            c.set_instance_transform(inst, m.reshape(16)); t0 = time.time(); c.commit(); tr.append((time.time() - t0) * 1e3)
        up, cm = [], []
        for k in range(6):
            new = [(m, wave(sc.meshes[m][0], 0.01, 0.5 * (k + 1))) for m in meshes]
            t0 = time.time()
            for m, v in new:
                c.update_mesh_vertices(m, v)
            t1 = time.time(); c.commit(); t2 = time.time()
            up.append((t1 - t0) * 1e3); cm.append((t2 - t1) * 1e3)
        t0 = time.time(); cost = c.tree_cost(); t_cost = (time.time() - t0) * 1e3
        ok = c.validate_bvh() if ntri < 1000000 else 0
        say(f"{tag:26s}: transform refit {med(tr[1:]):7.3f} | update {med(up):8.3f}  commit first {cm[0]:8.3f}  then {med(cm[1:]):8.3f} | tree_cost() {t_cost:6.3f} ms -> {cost[0]:.2f} / {cost[1]:.2f} | valid {ok}")
        if not tag.startswith("host refit"):
            c.set_option(rt.OPT_DEFORM_REBUILD, 1)
            rb = []
            for k in range(2):
                for m in meshes:
                    c.update_mesh_vertices(m, wave(sc.meshes[m][0], 0.01, 4.0 + k))
                t0 = time.time(); c.commit(); rb.append((time.time() - t0) * 1e3)
            say(f"{'':26s}  RTX_OPT_DEFORM_REBUILD 1 commit {min(rb):9.2f}")
        c.close()
    say()
say("```")
say()

# ---- 30 steps of a growing deformation of the 262 k atrium: what a threshold would be chosen from ----
say("## 30 steps of a growing wave over the 262 k atrium, 1280 x 720, 1 spp, 3 bounces: per step the commit, the frame (rtx_stats.render_ms) and the tree cost now / after the build")
say()
say("```")
sc = Arrays(rt.Scene.sponza_class())
W, H = 1280, 720
p = rt.Params(width=W, height=H, spp=1, max_bounces=3, nee_samples=1, flags=0)
for tag, policy in (("refit only (0)", 0), ("rebuild every step (1), GPU builder", 1)):
    c = rt.Context(0); c.set_option(rt.OPT_GPU_BUILD, 1); c.set_option(rt.OPT_DEFORM_REBUILD, policy); c.upload(sc, W / H)
    c.clear(W, H); c.render(p); base_ms = c.stats().render_ms
    rows = []
    for k in range(1, 31):
        for m in range(len(sc.meshes)):
            c.update_mesh_vertices(m, wave(sc.meshes[m][0], 0.004 * k, 0.3 * k))
        t0 = time.time(); c.commit(); t_c = (time.time() - t0) * 1e3
        c.clear(W, H); c.render(p)
        cost = c.tree_cost() if k in (1, 5, 10, 20, 30) else None
        rows.append((k, t_c, c.stats().render_ms, cost))
    say(f"{tag}: undeformed frame {base_ms:.2f} ms; commit median {med([r[1] for r in rows]):.2f} ms, frame median {med([r[2] for r in rows]):.2f} ms, commit + frame {med([r[1] + r[2] for r in rows]):.2f} ms")
    for k, t_c, fr_ms, cost in rows:
        if cost:
            say(f"    step {k:2d}: commit {t_c:7.2f}  frame {fr_ms:6.2f}  cost {cost[0]:.2f} / {cost[1]:.2f} = {100.0 * cost[0] / cost[1]:.1f} %")
    c.close()
say("```")
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")

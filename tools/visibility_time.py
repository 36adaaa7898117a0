"""Wall time of visibility commits (rtx_set_instance_visible + rtx_commit_scene) beside (a) the transform-only partial refit of the same instance on the same library and
(b) the route a caller had before: the scene re-added WITHOUT the instance and committed in a fresh context (host builder and RTX_OPT_GPU_BUILD; measured with --parent-pkg
on the parent commit's built package directory, in a child process — one process holds one library).  Then what the hidden instance still costs a frame: frame time and
work per ray of the scene with the instance hidden against a fresh context built without it.
    python tools/visibility_time.py [--parent-pkg DIR/royaltracer-dx_amd] [--out profiles/visibility_time.md] [--no-street] [--paste FILE ...]"""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--parent-pkg", default="", help="the parent commit's royaltracer-dx_amd directory with its librtx_hip.so built")
ap.add_argument("--out", default="")
ap.add_argument("--no-street", action="store_true")
ap.add_argument("--paste", nargs="*", default=[], help="text files appended verbatim (the bench.py lines of this commit and of its parent)")
ap.add_argument("--fresh-only", default="", help="(child process) case name: print the fresh-context times as JSON and exit")
args = ap.parse_args()

import __graft_entry__ as g
if args.fresh_only and args.parent_pkg:
    g.PKG_DIR = os.path.abspath(args.parent_pkg)            # (child process: the parent commit's package and library)
rt = g.load_package()
GOLD = os.path.join(ROOT, "tests", "golden")


def place(x, y, z, s):
    m = np.eye(4, dtype=np.float32); m[0, 0] = m[1, 1] = m[2, 2] = s; m[3, 0], m[3, 1], m[3, 2] = x, y, z
    return m.reshape(16)


def facing_x(x, y, z, s):
    """a panel of the xy plane turned into the yz plane (local x -> world z, local z -> world -x), scaled and placed"""
    m = np.zeros((4, 4), np.float32); m[0, 2] = s; m[1, 1] = s; m[2, 0] = -s; m[3] = (x, y, z, 1.0)
    return m.reshape(16)


def grid_mesh(n, size, base, mat):
    """n x n quads in the xy plane (a facade panel, a lamp): (verts (.., 7), indices, material ids)"""
    g1 = n + 1
    gx, gy = np.meshgrid(np.linspace(-size, size, g1), np.linspace(-size, size, g1), indexing="ij")
    v = np.zeros((g1 * g1, 7), np.float32); v[:, 0], v[:, 1], v[:, 6] = gx.ravel(), gy.ravel(), float(base)
    q = (np.arange(n)[:, None] * g1 + np.arange(n)[None, :]).ravel()
    idx = np.stack([q, q + g1, q + 1, q + 1, q + g1, q + g1 + 1], 1).ravel().astype(np.uint32)
    return v, idx, np.full(len(idx), mat, np.uint32)


class Arrays:
    """a big one-mesh scene plus small instances appended behind it: extras = [(name, 'monke' | 'lamp' (an emissive grid) | 'panel' (a 2048-triangle facade panel), transform)]"""
    def __init__(self, big, extras):
        self.materials = np.asarray(big.materials, np.float32); self.meshes = list(big.meshes); self.instances = list(big.instances); self._big = big
        self.names = {}
        base = sum(len(m) for _, _, m in big.meshes)
        lamp = np.array(self.materials[np.argmax(self.materials[:, 8:11].sum(1))], np.float32, copy=True); lamp[8:11] = (6.0, 5.0, 4.0)
        dull = int(np.argmin(self.materials[:, 8:11].sum(1)))
        for name, what, o2w in extras:
            if what == "monke":
                small = rt.Scene.from_obj([os.path.join(GOLD, "monke.obj")], GOLD + "/")
                nm = len(self.materials); self.materials = np.concatenate([self.materials, np.asarray(small.materials, np.float32)])
                v, i, m = small.meshes[0]
                v = np.array(v, np.float32, copy=True).reshape(-1, 7); v[:, 6] = float(base)
                mesh = (v, i, np.asarray(m, np.uint32) + np.uint32(nm))
            elif what == "lamp":
                self.materials = np.concatenate([self.materials, lamp[None]]); mesh = grid_mesh(6, 0.15, base, len(self.materials) - 1)
            else:
                mesh = grid_mesh(32, 1.0, base, dull)
            base += len(mesh[2])
            self.meshes.append(mesh); self.names[name] = len(self.instances); self.instances.append((len(self.meshes) - 1, o2w))
    def view_proj(self, aspect): return self._big.view_proj(aspect)
    def without(self, inst):
        s = Arrays.__new__(Arrays); s.materials, s.meshes, s._big = self.materials, self.meshes, self._big
        s.instances = [x for k, x in enumerate(self.instances) if k != inst]
        return s


def cases():
    yield "262 k atrium", (lambda: Arrays(rt.Scene.sponza_class(), [("monke", "monke", place(0.0, 0.3, 0.0, 0.25)), ("lamp (emits)", "lamp", place(-0.6, 1.1, 0.0, 1.0))]))
    if not args.no_street:
        yield "3.8 M street", (lambda: Arrays(rt.Scene.bistro_class(), [("facade panel", "panel", facing_x(0.5, 0.6, 0.0, 0.4))]))


def fresh_times(sc):
    """the scene handed over and committed in a new context: the only route to a scene without the instance before rtx_set_instance_visible"""
    out = {}
    for tag, gb in (("host builder", 0), ("RTX_OPT_GPU_BUILD", 1)):
        ts = []
        for k in range(2):
            c = rt.Context(0); c.set_option(rt.OPT_GPU_BUILD, gb); t0 = time.time(); c.upload(sc, 16 / 9); ts.append((time.time() - t0) * 1e3); c.close()
        out[tag] = min(ts)
    return out


if args.fresh_only:
    case, inst_name = args.fresh_only.split("|")
    for name, make in cases():
        if name == case:
            sc = make()
            print("FRESH " + json.dumps(fresh_times(sc.without(sc.names[inst_name]))))
    sys.exit(0)

lines = []
def say(s=""):
    print(s, flush=True); lines.append(s)

med = lambda a: float(np.median(a))
W, H = 1920, 1080
P = rt.Params(width=W, height=H, spp=4, max_bounces=8, nee_samples=1, flags=0)


def frame(c):
    """median frame time of 5 frames (rtx_stats.render_ms), then node steps / triangle tests per ray of one more frame with the counters on"""
    ms = []
    for k in range(6):
        c.clear(W, H); c.render(P); ms.append(c.stats().render_ms)
    c.set_option(rt.OPT_TRACE_COUNTERS, 1); c.trace_counters(); c.clear(W, H); c.render(P)
    st, cnt = c.stats(), c.trace_counters()
    c.set_option(rt.OPT_TRACE_COUNTERS, 0)
    nc, na = max(1, st.rays_primary + st.rays_extension), max(1, st.rays_shadow)
    return med(ms[1:]), (cnt[0] / nc, cnt[1] / nc, cnt[2] / na, cnt[3] / na)


say("# Visibility commits (tools/visibility_time.py): wall time of rtx_set_instance_visible + rtx_commit_scene")
say()
say("env: " + " ".join(f"{k}={os.environ[k]}" for k in sorted(os.environ) if k.startswith(("HIP_", "HSA_", "GPU_", "ROCR_", "OMP_NUM"))) + " | fresh-context rows measured on " + ("the parent commit's library" if args.parent_pkg else "THIS library (no --parent-pkg)"))
say()
say("One box, one process per library.  Commit times in ms, wall clock around rtx_commit_scene (it ends with a stream synchronise): the median of 5 after one discarded.  `transform` = (a), the")
say("transform-only partial refit of the same instance; `hide` / `show` = the commit after rtx_set_instance_visible(inst, 0 / 1).  `fresh` = (b), re-add the scene without the instance and")
say("commit it in a new context (minimum of 2).  Frames: 1920 x 1080, 4 spp, 8 bounces, NEE 1, rtx_stats.render_ms, the median of 5 after one discarded; work per ray = node steps and")
say("triangle tests per closest-hit ray | per any-hit ray (RTX_OPT_TRACE_COUNTERS, a frame of its own).")
say()
say("```")
for name, make in cases():
    sc = make()
    ntri = sum(len(sc.meshes[m][1]) // 3 for m, _ in sc.instances)
    say(f"== {name}: {ntri} triangles ==")
    for inst_name, inst in sc.names.items():
        say(f"-- instance {inst}: {inst_name}, {len(sc.meshes[sc.instances[inst][0]][1]) // 3} triangles --")
        if args.parent_pkg:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fresh-only", name + "|" + inst_name, "--parent-pkg", args.parent_pkg] + (["--no-street"] if args.no_street else []), capture_output=True, text=True, timeout=900)
            got = [l for l in p.stdout.splitlines() if l.startswith("FRESH ")]
            fr = json.loads(got[0][6:]) if p.returncode == 0 and got else {}
            if not fr:
                say("fresh context on the parent's library: FAILED " + p.stderr[-300:])
        else:
            fr = fresh_times(sc.without(inst))
        for tag, ms in fr.items():
            say(f"fresh context without it, re-add + commit, {tag:18s}: {ms:9.2f}")
        for tag, opts in (("host-built tree", []), ("GPU-built tree", [(rt.OPT_GPU_BUILD, 1)])):
            c = rt.Context(0)
            for o, v in opts:
                c.set_option(o, v)
            c.upload(sc, W / H)
            tr, hide, show = [], [], []
            for k in range(6):
                m = np.array(sc.instances[inst][1], np.float32, copy=True).reshape(4, 4); m[3, 1] += 0.01 * (k + 1)
                c.set_instance_transform(inst, m.reshape(16)); t0 = time.time(); c.commit(); tr.append((time.time() - t0) * 1e3)
            for k in range(6):
                c.set_instance_visible(inst, False); t0 = time.time(); c.commit(); hide.append((time.time() - t0) * 1e3)
                c.set_instance_visible(inst, True); t0 = time.time(); c.commit(); show.append((time.time() - t0) * 1e3)
            assert c.stats().bvh_refits == 18
            ok = c.validate_bvh() if ntri < 1000000 else 0
            say(f"{tag:16s}: transform {med(tr[1:]):7.3f} | hide {med(hide[1:]):7.3f} | show {med(show[1:]):7.3f} | valid {ok}")
            if inst == max(sc.names.values()):                  # once per scene and tree: what the hidden instance still costs a frame
                c.set_instance_transform(inst, sc.instances[inst][1]); c.set_instance_visible(inst, False); c.commit()
                ms_h, w_h = frame(c)
                c.close()
                f = rt.Context(0)
                for o, v in opts:
                    f.set_option(o, v)
                f.upload(sc.without(inst), W / H)
                ms_f, w_f = frame(f)
                f.close()
                fmt = lambda w: f"{w[0]:.2f} / {w[1]:.2f} | {w[2]:.2f} / {w[3]:.2f}"
                say(f"{'':16s}  frame, instance hidden {ms_h:7.3f} ms, work per ray {fmt(w_h)}")
                say(f"{'':16s}  frame, built without it {ms_f:7.3f} ms, work per ray {fmt(w_f)}")
            else:
                c.close()
    say()
say("```")
for path in args.paste:
    say(); say(f"## {os.path.basename(path)}"); say(); say("```"); say(open(path).read().rstrip()); say("```")
if args.out:
    open(args.out, "w").write("\n".join(lines) + "\n")

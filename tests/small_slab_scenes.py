"""Tiny scenes for the slab form of the pre-test records (tests/test_small_slabs_ref.py on the CPU, tests/test_small_slabs.py on the GPU): written as OBJ files of explicit
triangles, so that the host layer builds them like any other scene, plus the float64 reference of a quad's bounding parallelogram and the rays aimed at corners and edges."""
import numpy as np

TAU = 0.02            # csrc/rtx_small_scene.cpp: kSlabTau
MTL = "newmtl wall\nKd 0.7 0.6 0.5\nnewmtl lamp\nKd 0 0 0\nKe 9 8 7\n"


def quad_excess(q):
    """q (4, 3) float64, a planar convex quad in order -> excess area of the smallest bounding parallelogram along two ADJACENT edge normals, as a fraction"""
    q = np.asarray(q, np.float64)
    n = np.cross(q[1] - q[0], q[2] - q[0]); n /= np.linalg.norm(n)
    m = []
    for k in range(4):
        e = np.cross(n, q[(k + 1) % 4] - q[k]); m.append(e / np.linalg.norm(e))
    area = 0.5 * abs(np.dot(np.cross(q[2] - q[0], q[3] - q[1]), n))
    best = np.inf
    for k in range(4):
        w = [np.ptp(q @ m[k]), np.ptp(q @ m[(k + 1) % 4])]
        s = abs(np.dot(np.cross(m[k], m[(k + 1) % 4]), n))
        if s > 1e-9:
            best = min(best, w[0] * w[1] / s / area - 1.0)
    return max(best, 0.0)


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def kite(eps):
    """the unit square in the plane z = 0.25 with one corner pushed out along the diagonal by eps (planar in float32 whatever eps is)"""
    return f32([[0, 0, 0.25], [1, 0, 0.25], [1 + eps, 1 + eps, 0.25], [0, 1, 0.25]])


def eps_for_excess(target):
    lo, hi = 0.0, 0.5
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if quad_excess(kite(mid)) < target else (lo, mid)
    return hi


class Shapes:
    """collects quads (two triangles sharing the diagonal 0-2) and triangles; the first shape added is the lamp"""
    def __init__(self):
        self.v, self.f, self.quads, self.nlamp = [], [], [], 0

    def quad(self, q):
        q = f32(q); b = len(self.v) + 1
        self.nlamp = self.nlamp or 2
        self.v.extend(q); self.f.extend([(b, b + 1, b + 2), (b, b + 2, b + 3)]); self.quads.append(q)
        return self

    def tri(self, t):
        b = len(self.v) + 1
        self.nlamp = self.nlamp or 1
        self.v.extend(f32(t)); self.f.append((b, b + 1, b + 2))
        return self

    def ntris(self):
        return len(self.f)

    def write(self, d, name):
        txt = ["mtllib slabs.mtl"] + ["v %.9g %.9g %.9g" % tuple(p) for p in self.v] + ["usemtl lamp"]
        for i, f in enumerate(self.f):
            if i == self.nlamp:
                txt.append("usemtl wall")
            txt.append("f %d %d %d" % f)
        (d / "slabs.mtl").write_text(MTL)
        (d / (name + ".obj")).write_text("\n".join(txt) + "\n")
        return [str(d / (name + ".obj"))], str(d) + "/"

    def corners(self):
        return np.asarray(self.v, np.float64)


def rect(rng, grid=64.0):
    """an EXACT rectangle: corner and edge vectors on a binary grid, a = (p, q, 0), b = (-q, p, s) k, so a . b = 0 without rounding"""
    while True:
        p, q, s = (int(x) for x in rng.integers(-12, 13, 3))
        if p * p + q * q:
            break
    a = np.array([p, q, 0.0]) / grid
    b = np.array([-q, p, s]) / grid * float(rng.integers(1, 3))
    perm = rng.permutation(3)
    a, b = a[perm], b[perm]
    c = np.round(rng.uniform(-0.7, 0.7, 3) * grid) / grid
    return [c, c + a, c + a + b, c + b]


def scene_rects(rng, n=24):
    s = Shapes()
    for _ in range(n):
        s.quad(rect(rng))
    return s


def scene_perturbed():
    """kites whose excess lies just below and just above TAU (and far on either side), a trapezoid, a triangle, a zero-area triangle"""
    s = Shapes().quad(f32([[0.3, 0.3, 0.9], [0.6, 0.3, 0.9], [0.6, 0.6, 0.9], [0.3, 0.6, 0.9]]))
    off = 0
    for target in (0.95 * TAU, 1.05 * TAU, 0.002, 0.2):
        k = kite(eps_for_excess(target)) * 0.4; k[:, 0] += off * 0.5 - 0.9; k[:, 1] -= 0.8; k[:, 2] = 0.125 * off
        s.quad(k); off += 1
    s.quad(f32([[-0.5, 0.2, -0.25], [0.5, 0.2, -0.25], [0.25, 0.7, -0.25], [-0.25, 0.7, -0.25]]))          # trapezoid: the top half as wide as the base
    s.quad(f32([[-0.75, -0.25, 0.5], [-0.25, -0.25, 0.5], [-0.3125, 0.25, 0.5], [-0.75, 0.3125, 0.5]]))    # a general convex quad
    s.tri(f32([[0.1, -0.2, -0.5], [0.7, -0.1, -0.4], [0.3, 0.5, -0.6]]))
    s.tri(f32([[0.2, 0.2, 0.2], [0.4, 0.4, 0.4], [0.3, 0.3, 0.3]]))                                          # zero area
    return s


def scene_records(rng, nrec):
    """nrec records within the 64-triangle limit: as many exact rectangles as fit, the rest single triangles (which never find a partner: no shared edge)"""
    nquad = min(nrec, 64 - nrec)
    s = Shapes()
    order = rng.permutation(nrec)
    for k in order:
        if k < nquad:
            s.quad(rect(rng))
        else:
            c = rng.uniform(-0.8, 0.8, 3)
            s.tri([c + rng.normal(scale=0.2, size=3) for _ in range(3)])
    return s


RECORD_COUNTS = (1, 2, 3, 31, 32, 33, 63, 64)


def random_rays(n, rng, lo=-1.2, hi=1.2, tmin=1e-4, tmax=1e4):
    r = np.zeros((n, 8), np.float32)
    r[:, 0:3] = rng.uniform(lo, hi, (n, 3)); d = rng.normal(size=(n, 3)); r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    r[:, 3], r[:, 7] = tmin, tmax
    return r


def aimed_rays(shapes, rng, per=12):
    """rays from random origins at the corners of every shape, at points on its edges, and — for quads — at points of the bounding box of the quad in its plane that
    lie outside the quad (where the slab form can accept what the edge form rejects)"""
    V = shapes.corners()
    targets = [V + rng.normal(scale=1e-6, size=V.shape) for _ in range(2)] + [V]
    for q in shapes.quads:
        for k in range(4):
            u = rng.uniform(0, 1, (per, 1)); targets.append(q[k] * (1 - u) + q[(k + 1) % 4] * u)
        c = q.mean(0)
        u = rng.uniform(-1.15, 1.15, (4 * per, 2))
        targets.append(c + u[:, :1] * (q[1] - q[0]) * 0.5 + u[:, 1:] * (q[3] - q[0]) * 0.5)
    T = np.concatenate(targets)
    T = np.repeat(T, 2, axis=0)
    o = T + rng.normal(size=T.shape) * rng.uniform(0.05, 1.5, (len(T), 1))
    d = T - o; dist = np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((len(T), 8), np.float32)
    r[:, 0:3] = o; r[:, 4:7] = d / dist; r[:, 3] = 1e-4; r[:, 7] = 1e4
    return r


def all_scenes(rt, d, seed=11):
    """name -> (rt.Scene, Shapes or None): Cornell, exact rectangles, the perturbed quads, and one scene per record count"""
    rng = np.random.default_rng(seed)
    out = {"cornell": (rt.Scene.cornell(), None)}
    for name, s in [("rects", scene_rects(rng)), ("perturbed", scene_perturbed())] + [("records%d" % n, scene_records(rng, n)) for n in RECORD_COUNTS]:
        assert s.ntris() <= 64
        out[name] = (rt.Scene.from_obj(*s.write(d, name)), s)
    return out

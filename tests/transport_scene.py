"""The scene of the transport energy tests (tests/test_transport_ref.py, tests/test_transport.py, tests/golden/make_transport_ref.py): 8 triangles.

  floor    y = 0, z in [0, 3.4], GGX material, map_Kd + normal map, MIRRORED UVs (negative determinant), rotated in the plane: not axis-aligned
  wall     z = 0, y in [0, 1.58], meets the floor at a right angle; GGX material, map_Kd + normal map, UVs rotated the other way; its own mesh, instanced with a rotation
           about a skew axis — and in the config `env+kd+nrm` with a mirroring as well (the object-space mesh is the pre-image, so the WORLD geometry and the world position
           of every texel are the same: a renderer that handles handedness gives the same image, one that does not gives another)
  emitter  a small quad overhead facing down, behind the camera's field of view (one triangle light pair, nee_samples = 1)
  card     a vertical cut-out card beside the camera, outside its view, between the bright part of the sky and the floor: Kd = Ks = 0, an alpha blob that crosses 0.5 INSIDE
           the card
  sky      8 x 8 octahedral map, every upper-hemisphere texel lit, max / mean about 7, distinct per channel, rotated about Y (so `below the floor` stays `below`): every texel
           whose directions all have y < 0 is zero, and what a direction under the floor sees is no question (a texel the horizon runs through is lit on both sides of it: a
           continuation ray that leaves through its own floor finds that light, on the device as in the twin, and a shadow ray does not — see transport_ref's docstring)
  camera   pinhole, no yaw and no roll: the seam and the wall's top edge are horizontal lines of the image, and the pitch puts both between two rows of pixel rays

Sizes are the smallest that separate the wrong variants of transport_ref.WRONG (the power check of test_transport_ref.py), not chosen by eye."""
import math

import numpy as np

W, H, EDGE = 32, 24, 4
ASPECT = W / H
FOV_DEG = 45.0
EYE, CENTER = (0.0, 1.5, 3.3), (0.0, 0.62, 0.0)
WALL_HEIGHT = 1.58                                                # between the hit heights of pixel-ray rows 3 and 4: block row 0 is sky
SEAM_MARGIN = 0.03                                                # a shaded pixel closer than this (world units) to the seam or to a quad edge puts its block out
CONFIGS = ("env", "env+kd", "env+kd+nrm", "env+kd+nrm+cut", "kd+nrm")
MAX_BOUNCES = (1, 2, 3)
# the GPU test's sample counts: K frames of SPP samples each (sized by the power check); the fixture's n per pixel
GPU_FRAMES, GPU_SPP = 64, 1024
N_GPU = GPU_FRAMES * GPU_SPP
N_REF = 65536

FLOOR, WALL, EMITTER, CARD = 0, 1, 2, 3
KD_TEX, NRM_TEX, ALPHA_TEX = 0, 1, 2


def material(rt, kd, ks, rough, metal, ke=(0.0, 0.0, 0.0)):
    m = np.zeros(32, np.float32)
    m[0:3] = kd; m[3] = 1.0; m[4:7] = ks; m[7] = 1.0; m[8:11] = ke; m[12] = rough; m[13] = metal
    m[16:32] = rt.generate_ess_lut(rough)
    return m


def rotation(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    t = math.radians(deg)
    return np.eye(3) + math.sin(t) * K + (1.0 - math.cos(t)) * (K @ K)


def mat16(M3):
    m = np.eye(4)
    m[:3, :3] = M3
    return m.T.astype(np.float32).reshape(16)                     # element (r, c) at m[c * 4 + r]


def quad(p0, e1, e2, normal, to_object=None):
    """four vertices p0, p0 + e1, p0 + e1 + e2, p0 + e2 with one normal; to_object (3, 3): the mesh holds the pre-image of the world quad"""
    p = np.array([p0, np.add(p0, e1), np.add(np.add(p0, e1), e2), np.add(p0, e2)], np.float64)
    n = np.tile(np.asarray(normal, np.float64), (4, 1))
    if to_object is not None:
        p, n = p @ to_object.T, n @ to_object.T
    v = np.zeros((4, 7), np.float32)
    v[:, :3], v[:, 3:6] = p, n
    return v


def affine_uv(world4, origin, A):
    """uv = A (x - origin) on the quad's WORLD corners, picked to two of the three coordinates by A (2, 3); per index entry (0, 1, 2, 0, 2, 3)"""
    uv = (np.asarray(world4, np.float64) - origin) @ np.asarray(A, np.float64).T
    return uv[[0, 1, 2, 0, 2, 3]].astype(np.float32)


def kd_texture():
    """16 x 16, smooth and non-block: a slow gradient plus a wave of period 4 texels, distinct per channel"""
    n = 16
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    px = np.full((n, n, 4), 255, np.uint8)
    for k, (fx, fy, ph) in enumerate(((1, 0, 0.0), (0, 1, 1.3), (1, 1, 2.1))):
        slow = 0.5 + 0.22 * np.sin(2.0 * np.pi * (fx * x + fy * y) / n + ph)
        fast = 0.25 * np.sin(2.0 * np.pi * (x * (k + 1) + y * (3 - k)) / 4.0 + ph)
        px[..., k] = np.clip(np.round(255.0 * (slow + fast)), 20, 250)
    return px


def normal_texture():
    """32 x 32, smooth, tilts up to about 35 degrees in r and in g, no flat texel (r = g = 128 nowhere)"""
    n = 32
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    tx = 0.62 * np.sin(2.0 * np.pi * (x + 0.5 * y) / n + 0.4)
    ty = 0.62 * np.cos(2.0 * np.pi * (y - 0.25 * x) / n * 2.0 + 0.9) * 0.8 + 0.12
    c = np.stack([tx, ty, np.ones_like(tx)], -1)
    c /= np.linalg.norm(c, axis=-1, keepdims=True)
    px = np.full((n, n, 4), 255, np.uint8)
    px[..., :3] = np.clip(np.floor(c * 127.0 + 128.5), 0, 255)
    flat = (px[..., 0] == 128) & (px[..., 1] == 128)
    px[..., 0][flat] = 131
    return px


def alpha_texture():
    """16 x 16: a smooth blob, alpha about 1 in the middle and 0 at the border, crossing 0.5 well inside"""
    n = 16
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    r2 = ((x - 7.5) / 7.5) ** 2 + ((y - 7.5) / 7.5) ** 2
    px = np.zeros((n, n, 4), np.uint8)
    px[..., 3] = np.clip(np.round(255.0 * np.exp(-r2 / 0.35)), 0, 255)
    return px


def sky(strict=False):
    """8 x 8 octahedral map and its rotation about Y.  Upper hemisphere = the inner diamond |a| + |b| <= 1: a texel with a corner in it is lit (smoothly varying, per channel), a
    bright patch low over -x / +z; texels wholly outside (all directions y < 0) are zero.  strict: the texels the horizon runs through are zero as well — the sky of the
    reduced scene, where the textbook integral is the reference and a continuation ray that leaves through its own floor must find nothing"""
    n = 8
    img = np.zeros((n, n, 3), np.float32)
    for j in range(n):
        for i in range(n):
            corners = [(2.0 * (i + di) / n - 1.0, 2.0 * (j + dj) / n - 1.0) for di in (0, 1) for dj in (0, 1)]
            if min(abs(a) + abs(b) for a, b in corners) >= 1.0 or (strict and max(abs(a) + abs(b) for a, b in corners) > 1.0):
                continue
            a, b = 2.0 * (i + 0.5) / n - 1.0, 2.0 * (j + 0.5) / n - 1.0
            base = 0.45 + 0.2 * a - 0.15 * b
            img[j, i] = (base * 1.1, base, base * (0.8 + 0.3 * (b + 1.0) / 2.0) * 1.2)
    img[5, 1] = (5.2, 4.4, 3.2); img[5, 2] = (3.9, 3.4, 2.6); img[4, 1] = (2.6, 2.4, 2.0)
    return img, mat16(rotation((0.0, 1.0, 0.0), 25.0))


class TransportScene:
    """duck-typed for Context.upload, Oracle.load and transport_ref.Twin"""
    def view_proj(self, aspect):
        return self._view, self._proj


def build(rt, config, floor_only=False):
    """config: one of CONFIGS.  floor_only: floor + card (+ environment), no wall, no emitter — the reduced scene of the Lambert pair check"""
    assert config in CONFIGS
    parts = config.split("+")
    s = TransportScene()
    s.config, s.width, s.height, s.aspect, s.nee_samples = config, W, H, ASPECT, 1
    s.materials = np.stack([material(rt, (0.72, 0.66, 0.58), (0.06, 0.05, 0.04), 0.5, 0.25),
                            material(rt, (0.55, 0.68, 0.74), (0.05, 0.06, 0.08), 0.45, 0.3),
                            material(rt, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.5, 0.0, ke=(24.0, 20.0, 16.0)),
                            material(rt, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0.5, 0.0)])
    floor_w = quad((-2.4, 0.0, 0.0), (0.0, 0.0, 3.4), (4.8, 0.0, 0.0), (0.0, 1.0, 0.0))
    emit_w = quad((0.25, 2.3, 2.2), (0.5, 0.0, 0.0), (0.0, 0.0, 0.5), (0.0, -1.0, 0.0))
    card_w = quad((-1.25, 0.12, 1.45), (0.0, 0.0, 1.7), (0.0, 1.75, 0.0), (1.0, 0.0, 0.0))
    wall_w = quad((-2.4, 0.0, 0.0), (4.8, 0.0, 0.0), (0.0, WALL_HEIGHT, 0.0), (0.0, 0.0, 1.0))
    # UVs: affine in world position, rotated in the plane; the floor's have a negative determinant (mirrored)
    cf, sf = math.cos(math.radians(28.0)), math.sin(math.radians(28.0))
    floor_uv = affine_uv(floor_w[:, :3], (-2.4, 0.0, 0.0), 0.36 * np.array([[cf, 0.0, sf], [-sf, 0.0, cf]]))
    cw, sw = math.cos(math.radians(-17.0)), math.sin(math.radians(-17.0))
    wall_uv = affine_uv(wall_w[:, :3], (-2.4, 0.0, 0.0), 0.41 * np.array([[cw, -sw, 0.0], [sw, cw, 0.0]]))
    card_uv = affine_uv(card_w[:, :3], (-1.25, 0.12, 1.45), np.array([[0.0, 0.0, 1.0 / 1.7], [0.0, 1.0 / 1.75, 0.0]]))
    emit_uv = np.zeros((6, 2), np.float32)
    Rw = rotation((1.0, 2.0, 3.0), 40.0)
    if config == "env+kd+nrm":
        Rw = Rw @ np.diag([-1.0, 1.0, 1.0])                       # ... and a mirroring
    wall_o = quad((-2.4, 0.0, 0.0), (4.8, 0.0, 0.0), (0.0, WALL_HEIGHT, 0.0), (0.0, 0.0, 1.0), to_object=np.linalg.inv(Rw))
    six = np.array([0, 1, 2, 0, 2, 3], np.uint32)
    if floor_only:
        v0 = np.concatenate([floor_w, card_w]); mids = np.repeat(np.array([FLOOR, CARD], np.uint32), 6)
        uv0 = np.concatenate([floor_uv, card_uv])
    else:
        v0 = np.concatenate([floor_w, emit_w, card_w]); mids = np.repeat(np.array([FLOOR, EMITTER, CARD], np.uint32), 6)
        uv0 = np.concatenate([floor_uv, emit_uv, card_uv])
    i0 = np.concatenate([six + 4 * q for q in range(len(v0) // 4)]).astype(np.uint32)
    s.meshes, s.uvs = [(v0, i0, mids)], [uv0]
    s.instances = [(0, np.eye(4, dtype=np.float32).reshape(16))]
    if not floor_only:
        wall_o[:, 6] = float(len(i0))                             # Vertex.normal.w = the mesh's base in the scene's materialIDs
        s.meshes.append((wall_o, six.copy(), np.full(6, WALL, np.uint32))); s.uvs.append(wall_uv)
        s.instances.append((1, mat16(Rw)))
    s.textures = [(kd_texture(), True), (normal_texture(), False), (alpha_texture(), False)]
    none = [-1, -1, -1, -1]
    s.material_maps = [KD_TEX, KD_TEX, -1, -1] if "kd" in parts else list(none)
    s.normal_maps = [NRM_TEX, NRM_TEX, -1, -1] if "nrm" in parts else list(none)
    s.opacity_maps = [-1, -1, -1, ALPHA_TEX] if "cut" in parts else list(none)
    s.environment = None
    if "env" in parts:
        img, rot = sky(strict=floor_only)
        s.environment = dict(img=img, to_world=rot, scale=1.0)
    s._view = rt.lookat(EYE, CENTER, (0.0, 1.0, 0.0))
    s._proj = rt.perspective_fov_rh(math.radians(FOV_DEG), ASPECT, 0.1, 100.0)
    return s


def primary_rays(orc, rt, scene):
    """(W * H, 8) float32 rays of the oracle's ray generation: pixel corners, no jitter, so all samples of a pixel share one ray"""
    return orc.Oracle().load(scene, scene.aspect).primary_rays(rt.Params(width=W, height=H, spp=1, max_bounces=1, nee_samples=1))


class Blocks:
    """which 4 x 4 blocks carry statistics: every pixel shaded (hits the floor or the wall), no pixel within SEAM_MARGIN of the seam or of a quad's edge"""
    def __init__(self, twin, rays):
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 4:7].astype(np.float64)
        hq, ht, ha, hb = twin.closest(o, d, np.full(len(o), -1, np.int64))
        self.hq = hq.reshape(H, W)
        shaded = np.zeros(len(o), bool)
        clean = np.zeros(len(o), bool)
        for qi, Q in enumerate(twin.quads):
            sel = hq == qi
            if Q.emits:
                continue
            shaded |= sel
            ea, eb = np.minimum(ha, 1.0 - ha) * np.linalg.norm(Q.E1), np.minimum(hb, 1.0 - hb) * np.linalg.norm(Q.E2)
            clean |= sel & (np.minimum(ea, eb) >= SEAM_MARGIN)
        self.miss = (hq == -1).reshape(H, W)
        sh = shaded.reshape(H // EDGE, EDGE, W // EDGE, EDGE)
        cl = clean.reshape(H // EDGE, EDGE, W // EDGE, EDGE)
        self.any_shaded = sh.any(axis=(1, 3))
        self.used = cl.all(axis=(1, 3))
        self.left_out = self.any_shaded & ~self.used
        self.ids = [(int(bx), int(by)) for by, bx in zip(*np.nonzero(self.used))]

    def fraction_left_out(self):
        return float(self.left_out.sum()) / float(self.any_shaded.sum())


def block_means(img):
    """(H, W, C) -> (H / 4, W / 4, C) float64 means"""
    a = np.asarray(img, np.float64)
    return a.reshape(H // EDGE, EDGE, W // EDGE, EDGE, -1).mean(axis=(1, 3))


def tolerance(sigma_ref, mean_ref, n_gpu=N_GPU, n_ref=N_REF, spp=GPU_SPP):
    """6 sigma_ref sqrt(1 / n_gpu + 1 / n_ref) + spp 2^-24 |mean_ref|: six combined standard errors (the project's convention, tests/test_env.py) plus the bound of the
    sequential float32 accumulation of spp terms, the only systematic allowance"""
    return 6.0 * sigma_ref * math.sqrt(1.0 / n_gpu + 1.0 / n_ref) + spp * 2.0 ** -24 * np.abs(mean_ref)

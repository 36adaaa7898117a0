"""The float32 emulator of rtx_render_adaptive that tests/test_adaptive.py holds the GPU to, bit for bit, and the CPU test that its inputs are not vacuous.

An adaptively sampled image is predictable from the CPU oracle as it stands: seeds depend on pixel and sample id only, and the device adds a pixel's samples in sample order.
So the emulator takes PER-SAMPLE oracle frames (Oracle.render with spp = 1 and sample_base = b + n), the chunk geometry from sharding.slot_pixels, and replays the passes with
the criterion of include/rtx.h and sequential float32 additions:

    d = (|a.x - (h.x + h.x)| + |a.y - (h.y + h.y)|) + |a.z - (h.z + h.z)|
    s = (a.x + a.y) + a.z
    pixel converged  <=>  d * d < ((threshold * threshold) * max(s, dark_floor * N)) * N          (a = u1, h = sum of the odd sample ids, N = a.w)
"""
import functools
import numpy as np

import __graft_entry__ as graft

F = np.float32
# ---- the inputs of the GPU tests (tests/test_adaptive.py) ----
W, H, ASPECT = 100, 50, 2.0                   # neither side a multiple of 8: blocks hold invalid slots; at tile_size 32 whole chunks lie below the image
BASE = dict(width=W, height=H, sample_base=5, frame_seed=99, max_bounces=8, nee_samples=1)
MIN_SPP, STEP_SPP, MAX_SPP = 4, 4, 16
# Chosen here, on the CPU, from the oracle alone (test_inputs_are_not_vacuous prints the counts): with 0.25 the Cornell box at 100 x 50 has converged chunks (the
# surroundings of the box, flat wall strips) and open ones after 4, 8 and 12 samples, and chunks that end at 4, 8, 12 and 16 samples — at tile_size 16 and 32, with and
# without jitter (28 chunks with pixels each; e.g. tile 16 without jitter: 14, 18, 20, 22 converged after the four passes, 6 unconverged at the cap).
THRESHOLD = 0.25
TILES = (16, 32)


@functools.lru_cache(maxsize=None)
def oracle_frames(flags, nsamples=MAX_SPP):
    """frames[n] = the oracle's image (H, W, 4) of sample id sample_base + n alone; computed once per flag word and shared (read-only)"""
    rt, orc = graft.load_package(), graft.load_oracle()
    o = orc.Oracle().load(rt.Scene.cornell(), ASPECT)
    out = []
    for n in range(nsamples):
        img, _ = o.render(rt.Params(**dict(BASE, spp=1, flags=flags, sample_base=BASE["sample_base"] + n)))
        img.setflags(write=False)
        out.append(img)
    return tuple(out)


def chunk_geometry(width, height, tile_size, rank=0, world=1, blocks=False):
    """(x, y, valid), each (local chunks, 256): the pixels of the shard's 256-slot chunks"""
    graft.load_package()
    from royaltracer_dx_amd import sharding
    x, y, ok = sharding.slot_pixels(width, height, tile_size, rank, world, blocks)
    return x.reshape(-1, 256), y.reshape(-1, 256), ok.reshape(-1, 256)


class Emulation:
    """u1, half and the per-chunk words of one (unsharded or sharded) image; render_adaptive() replays one rtx_render_adaptive call on them"""

    def __init__(self, width, height, tile_size, rank=0, world=1, blocks=False):
        self.x, self.y, self.ok = chunk_geometry(width, height, tile_size, rank, world, blocks)
        self.accum = np.zeros((height, width, 4), F)
        self.half = np.zeros((height, width, 4), F)
        n = len(self.x)
        self.count = np.zeros(n, np.int64)
        self.flag = np.where(self.ok.any(1), 0, 2)             # 0 sampling, 1 converged, 2 no valid pixel
        self.converged_after_pass = []                          # chunks converged at every evaluation of the criterion, over all calls

    def _evaluate(self, threshold, dark_floor):
        t, df = F(threshold), F(dark_floor)
        for c in np.nonzero(self.flag == 0)[0]:
            ok = self.ok[c]
            a, h = self.accum[self.y[c][ok], self.x[c][ok]], self.half[self.y[c][ok], self.x[c][ok]]
            N = a[:, 3]
            d = (np.abs(a[:, 0] - (h[:, 0] + h[:, 0])) + np.abs(a[:, 1] - (h[:, 1] + h[:, 1]))) + np.abs(a[:, 2] - (h[:, 2] + h[:, 2]))
            s = (a[:, 0] + a[:, 1]) + a[:, 2]
            conv = d * d < ((t * t) * np.maximum(s, df * N)) * N
            assert d.dtype == F and conv.dtype == bool and (((t * t) * np.maximum(s, df * N)) * N).dtype == F
            if conv.all():
                self.flag[c] = 1

    def _add(self, chunks, frames, first, nsamples, base_is_odd):
        """samples first .. first + nsamples - 1 (indices into frames), in order, for every valid pixel of `chunks`"""
        ok = self.ok[chunks]
        ys, xs = self.y[chunks][ok], self.x[chunks][ok]
        a, h = self.accum[ys, xs], self.half[ys, xs]
        for n in range(first, first + nsamples):
            fr = frames[n][ys, xs]
            fin = fr[:, 3] == 1.0                              # the oracle, like k_accumulate, skips a non-finite sample: its frame keeps count 0 there
            a[fin, :3] = a[fin, :3] + fr[fin, :3]; a[fin, 3] = a[fin, 3] + F(1)
            if (n & 1) != base_is_odd:                         # sample id = base + n is odd
                h[fin, :3] = h[fin, :3] + fr[fin, :3]; h[fin, 3] = h[fin, 3] + F(1)
        self.accum[ys, xs], self.half[ys, xs] = a, h
        self.count[chunks] += nsamples
        return int(ok.sum()) * nsamples

    def render_adaptive(self, frames, sample_base, min_spp, step_spp, max_spp, threshold, dark_floor=0.0):
        """-> dict(passes, chunks, chunks_converged, chunks_at_max, pixel_samples) of this call"""
        dark_floor = dark_floor or 0.01
        passes = samples = 0
        while True:
            self._evaluate(threshold, dark_floor)
            self.converged_after_pass.append(int((self.flag == 1).sum()))
            cand = (self.flag == 0) & (self.count < max_spp)
            if not cand.any():
                break
            cur = int(self.count[cand].min())
            active = np.nonzero(cand & (self.count == cur))[0]
            step = min_spp - cur if cur < min_spp else min(step_spp, max_spp - cur)
            samples += self._add(active, frames, cur, step, 1 - (sample_base & 1))
            passes += 1
        return dict(passes=passes, chunks=int((self.flag != 2).sum()), chunks_converged=int((self.flag == 1).sum()),
                    chunks_at_max=int(((self.flag == 0) & (self.count >= max_spp)).sum()), pixel_samples=samples)


def emulate(flags, tile_size, max_spp=MAX_SPP, threshold=THRESHOLD):
    e = Emulation(W, H, tile_size)
    res = e.render_adaptive(oracle_frames(flags), BASE["sample_base"], MIN_SPP, STEP_SPP, max_spp, threshold)
    return e, res


def test_inputs_are_not_vacuous():
    """the GPU tests' exact inputs, on the oracle alone: the criterion must split the chunks after the min_spp pass and after a later one, and chunks must end both at
    the cap and below it — otherwise bit parity with the emulation would say nothing about the criterion, the list or the continuation"""
    for flags in (1, 3):
        for ts in TILES:
            e, res = emulate(flags, ts)
            total, conv = res["chunks"], e.converged_after_pass
            print(f"flags {flags} tile {ts}: chunks {total}, converged after each evaluation {conv}, at max {res['chunks_at_max']}, samples {res['pixel_samples']}, counts {sorted(set(e.count))}")
            assert conv[0] == 0 and res["passes"] >= 3
            assert 0 < conv[1] < total, "after the min_spp pass"
            assert any(0 < k < total and k > conv[1] for k in conv[2:]), "after a later pass (and it converged something more)"
            assert (e.count[e.flag != 2] == MAX_SPP).any() and res["chunks_at_max"] >= 1, "no chunk ends at max_spp"
            assert (e.count[e.flag != 2] < MAX_SPP).any(), "no chunk ends below max_spp"
            assert (e.flag == 2).any() == (ts == 32), "tile_size 32 has chunks without a valid pixel, 16 has none"
            # threshold 0 converges nothing: every chunk takes max_spp samples, i.e. the plain sum of the frames
            z, rz = emulate(flags, ts, threshold=0.0)
            assert rz["chunks_converged"] == 0 and rz["pixel_samples"] == W * H * MAX_SPP and (z.accum[..., 3] <= MAX_SPP).all()

"""Writes tests/golden/transport_ref.npz: the float64 estimator twin (tests/transport_ref.py) run at full sample count on the scene of tests/transport_scene.py.

Per config, mode (0 = GGX, 1 = RTX_FLAG_LAMBERT_ONLY), max_bounces (1, 2, 3), 4 x 4 pixel block (row, column) and channel: the mean, the per-sample standard deviation of the
block statistic (one sample = the mean over the block's 16 pixels of one path each), the standard deviation of each half of the samples and the fourth central moment (the
tail check of tests/test_transport_ref.py); per config the blocks that carry statistics and a hash of the scene's arrays; n.  Blocks that carry none hold NaN.

Run by hand from the repository root (it needs the built package for the host's look-at / projection / Ess table and the oracle for the primary rays; no GPU):

    python tests/golden/make_transport_ref.py [n per pixel] [output file] [processes]

About an hour of CPU at the default n = transport_scene.N_REF, spread over the processes.  Seeds are fixed: the output is reproducible to the bit on one numpy version and
statistically (tests/test_transport_ref.py, fixture freshness) on any."""
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SEED = 20261020


def block_rng(ci, fi, bx, by):
    return np.random.default_rng([SEED, ci, fi, by, bx])


def job(args):
    ci, fi, n = args
    import __graft_entry__ as graft
    import transport_ref as tf
    import transport_scene as ts
    rt, orc = graft.load_package(), graft.load_oracle()
    scene = ts.build(rt, ts.CONFIGS[ci])
    rays = ts.primary_rays(orc, rt, scene)
    tw = tf.Twin(scene, tf.LAMBERT_ONLY if fi else 0)
    blocks = ts.Blocks(tf.Twin(scene), rays)
    shape = (len(ts.MAX_BOUNCES), ts.H // ts.EDGE, ts.W // ts.EDGE, 3)
    res = [np.full(shape, np.nan) for _ in range(5)]
    for bx, by in blocks.ids:
        x = tf.block_samples(tw, rays, tf.block_pixels(ts.W, bx, by), n, len(ts.MAX_BOUNCES), block_rng(ci, fi, bx, by))
        for m in range(len(ts.MAX_BOUNCES)):
            for r, v in zip(res, tf.moments(x[m])):
                r[m, by, bx] = v
    return ci, fi, res, blocks.used, tf.scene_hash(scene)


def main():
    import transport_scene as ts
    n = int(sys.argv[1]) if len(sys.argv) > 1 else ts.N_REF
    path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "transport_ref.npz")
    procs = int(sys.argv[3]) if len(sys.argv) > 3 else min(8, os.cpu_count() or 1)
    nc = len(ts.CONFIGS)
    shape = (nc, 2, len(ts.MAX_BOUNCES), ts.H // ts.EDGE, ts.W // ts.EDGE, 3)
    names = ("mean", "std", "std_a", "std_b", "m4")
    out = {k: np.full(shape, np.nan) for k in names}
    used = np.zeros((nc, ts.H // ts.EDGE, ts.W // ts.EDGE), bool)
    hashes = [""] * nc
    with multiprocessing.get_context("spawn").Pool(procs) as pool:
        for ci, fi, res, u, h in pool.imap_unordered(job, [(ci, fi, n) for ci in range(nc) for fi in range(2)]):
            for k, r in zip(names, res):
                out[k][ci, fi] = r
            used[ci], hashes[ci] = u, h
            print(ts.CONFIGS[ci], "lambert" if fi else "ggx", "done", flush=True)
    np.savez_compressed(path, n=np.int64(n), configs=np.array(ts.CONFIGS), used=used, scene_hash=np.array(hashes),
                        mean=out["mean"], m4=out["m4"], **{k: out[k].astype(np.float32) for k in ("std", "std_a", "std_b")})
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

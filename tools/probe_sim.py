"""Dev tool (CPU only): dependent round trips of the train-triple membership test (csrc/kge_sampler_device.h) on the bench's own
table -- the synthetic FB15k-shape train split, 2^20 slots -- for one slot per trip (set_contains) and aligned groups of 4 / 8 / 16
slots per trip (set_contains_wide<W>), per lane, per 64-lane wave and per 256-thread workgroup (a wave leaves the probe loop with
its slowest lane, a workgroup ends with its slowest wave).  32 768 random corruptions of train triples, one batch of the flagship.

  python tools/probe_sim.py [seed]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
M64 = (1 << 64) - 1
EMPTY = M64


def pack(h, r, t):
    return ((h & 0xFFFFFF) << 40) | ((r & 0xFFFF) << 24) | (t & 0xFFFFFF)


def mix64(x):
    x ^= x >> 30; x = x * 0xBF58476D1CE4E5B9 & M64
    x ^= x >> 27; x = x * 0x94D049BB133111EB & M64
    return x ^ (x >> 31)


def main():
    import bench
    seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    train = bench.synthetic_split(bench.E, bench.R, (bench.N_TRAIN,))[0]
    n_slots = 1 << max(4, int(np.ceil(np.log2(2 * len(train)))))
    mask = n_slots - 1
    slots = [EMPTY] * n_slots
    for h, r, t in train.tolist():
        k = pack(h, r, t)
        s = mix64(k) & mask
        while slots[s] != EMPTY and slots[s] != k:
            s = (s + 1) & mask
        slots[s] = k
    load = sum(v != EMPTY for v in slots) / n_slots
    rng = np.random.default_rng(seed)
    B = 32768
    pos = train[rng.integers(len(train), size=B)]
    ent = rng.integers(bench.E, size=B)
    tail = rng.random(B) > 0.5
    widths = (1, 4, 8, 16)
    trips = np.zeros((len(widths), B), dtype=np.int64)
    lines = np.zeros(B, dtype=np.int64)
    for i in range(B):
        h, r, t = pos[i].tolist()
        k = pack(h, r, int(ent[i])) if tail[i] else pack(int(ent[i]), r, t)
        home = mix64(k) & mask
        s, seen = home, 1
        while slots[s] != EMPTY and slots[s] != k:
            s = (s + 1) & mask
            seen += 1
        for wi, w in enumerate(widths):
            trips[wi, i] = (((home & (w - 1)) + seen - 1) // w) + 1
        lines[i] = (((home & 7) + seen - 1) // 8) + 1
    print("table: %d triples, %d slots, load %.3f; %d random corruptions (seed %d)" % (len(train), n_slots, load, B, seed))
    print("| probe form | per lane (mean) | per wave (mean / p90 / max) | per 256-thread workgroup (mean / max) |")
    print("|---|---|---|---|")
    for wi, w in enumerate(widths):
        wave = trips[wi].reshape(-1, 64).max(1)
        wg = trips[wi].reshape(-1, 256).max(1)
        print("| %s | %.2f | %.1f / %d / %d | %.1f / %d |" % ("one slot per trip" if w == 1 else "aligned group of %d" % w, trips[wi].mean(),
                                                            wave.mean(), int(np.percentile(wave, 90)), wave.max(), wg.mean(), wg.max()))
    print("64-byte lines a lane's probe touches: mean %.2f" % lines.mean())


if __name__ == "__main__":
    main()

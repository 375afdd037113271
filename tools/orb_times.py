"""Times of ba_orb_extract (output kept in profiles/orb_times.txt).

    python tools/orb_times.py [--out FILE] [--case N]

Host wall time of Solver.extract_orb (every output copied back and compacted), median of 11 after 3 warm-up calls, for 1, 4 and 16
images of 1280 x 720 at the default options (3000 features, 8 levels, scale 1.2), and the time of each stage of one such call
from events on the handle's stream (ba_orb_stage_times; the median over the same calls).  Images: synthetic texture -- seeded
random rectangles, blobs and noise, a different seed per image.  --case N runs one batch size alone (what a kernel trace of that
case is taken from).  Recorded, not gated: there is no CPU comparator on the build machine."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS, WARM = 11, 3
CASES = (1, 4, 16)
H, W = 720, 1280


def texture(h, w, seed, n_rect=900, noise=5):
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 110.0, dtype=np.float32)
    for _ in range(n_rect):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(4, 60)), x0:x0 + int(rng.integers(4, 60))] = float(rng.integers(0, 256))
    for _ in range(n_rect // 2):
        cx, cy, r = int(rng.integers(12, w - 12)), int(rng.integers(12, h - 12)), float(rng.uniform(2, 4))
        yy, xx = np.mgrid[cy - 12:cy + 12, cx - 12:cx + 12]
        img[cy - 12:cy + 12, cx - 12:cx + 12] += float(rng.uniform(-120, 120)) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
    img += rng.normal(0, noise, (h, w)).astype(np.float32)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_times.txt"))
    ap.add_argument("--case", type=int, default=-1)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    images = np.stack([texture(H, W, seed) for seed in range(max(CASES))])
    lines = []
    with hb.Solver(0) as s:
        s.orb_stage_times(enable=True)
        for case, n in enumerate(CASES):
            if a.case >= 0 and case != a.case:
                continue
            batch = np.ascontiguousarray(images[:n])
            for _ in range(WARM):
                out = s.extract_orb(batch)
            wall, stages = [], []
            for _ in range(REPS):
                t0 = time.perf_counter()
                s.extract_orb(batch)
                wall.append(time.perf_counter() - t0)
                stages.append(s.orb_stage_times())
            med = {k: float(np.median([st[k] for st in stages])) for k in stages[0]}
            lines.append(f"{n} image(s) of {W} x {H}, defaults: wall {1e3 * float(np.median(wall)):.3f} ms (min {1e3 * min(wall):.3f}, max "
                         f"{1e3 * max(wall):.3f}); keypoints per image {out['n_kp'].min()} .. {out['n_kp'].max()}; stages on the stream, ms: "
                         + ", ".join(f"{k} {v:.3f}" for k, v in med.items()) + f"; sum {sum(med.values()):.3f}")
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

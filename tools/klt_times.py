"""Times of ba_track_klt beside the per-frame stage it can stand in for (output kept in profiles/klt_times.txt).

    python tools/klt_times.py [--out FILE]

One pair of 1280 x 720 images, the second the first moved by (5, -3) pixels, 3000 points (the keypoints ba_orb_extract finds in
the first image), ba_track_klt at the defaults (21 x 21 window, 3 levels above the image, 30 iterations, eps 0.01):
  wall      host wall time of Solver.track_klt, every output copied back, median of 21 calls after 5 warm-up calls;
  stream    the stages of the same calls from events on the handle's stream (ba_klt_stage_times), median per stage;
  fb        the same with the forward-backward check (fb_max_px 1).
Next to it, on the same two images and the same handle: ba_orb_extract of the second image (3000 features, defaults) plus
ba_match_descriptors of the first image's descriptors against it -- what a front end that extracts and matches every frame
against the last keyframe spends per frame, where the tracker needs the new frame alone.  The ratio is (extract + match) / track,
wall over wall.  Images: the synthetic texture of tools/orb_times.py.  Recorded, not gated: nobody has measured this kernel
before, and there is no CPU comparator on the build machine."""
import argparse
import os
import platform
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 21, 5
H, W, N = 720, 1280, 3000
SHIFT = (5, -3)       # (dx, dy)


def timed(f):
    for _ in range(WARM):
        out = f()
    wall = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = f()
        wall.append(1e3 * (time.perf_counter() - t0))
    return out, wall


def fmt(wall):
    return f"{float(np.median(wall)):.3f} ms (min {min(wall):.3f}, max {max(wall):.3f})"


def device_name():
    """The name of device 0 from the HIP runtime the library itself runs on (call it with a handle open)."""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
        buf = C.create_string_buffer(256)
        if hip.hipDeviceGetName(buf, 256, 0) == 0 and buf.value:
            return buf.value.decode()
    except (OSError, AttributeError):      # the name is a label of the record, nothing depends on it
        pass
    return "device 0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "klt_times.txt"))
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    from orb_times import texture
    first = texture(H, W, 0)
    imgs = np.stack([first, np.roll(first, (SHIFT[1], SHIFT[0]), axis=(0, 1))])
    with hb.Solver(0) as s:
        lines = [f"{device_name()} on {platform.node()}; {REPS} calls after {WARM} warm-up calls, medians; one pair of {W} x {H}, the content moved by {SHIFT}"]
        kp = s.extract_orb(imgs[0], n_features=N)
        pts = kp["xy"]
        assert len(pts) == N, len(pts)
        s.klt_stage_times(enable=True)
        stages = []

        def track(**kw):
            out = s.track_klt(imgs, [(0, 1)], [pts], **kw)
            stages.append(s.klt_stage_times())
            return out

        walls = {}
        for name, kw in (("defaults", {}), ("defaults + forward-backward check (fb_max_px 1)", dict(fb_max_px=1.0))):
            del stages[:]
            out, wall = timed(lambda: track(**kw))
            med = {k: float(np.median([st[k] for st in stages[WARM:]])) for k in hb.KLT_STAGES}
            ok = out["status"] == hb.KLT_STATUS["ok"]
            miss = np.hypot(*(out["next"][ok].astype(np.float64) - pts[ok] - SHIFT).T)
            walls[name] = float(np.median(wall))
            lines.append(f"ba_track_klt, {N} points, {name}: wall {fmt(wall)}; stages on the stream, ms: "
                         + ", ".join(f"{k} {v:.3f}" for k, v in med.items()) + f"; sum {sum(med.values()):.3f}; {int(ok.sum())} of {N} OK, "
                         f"median miss of those {float(np.median(miss)):.3f} px")
            print(lines[-1], flush=True)
        s.klt_stage_times(enable=False)
        _, w_ext = timed(lambda: s.extract_orb(imgs[1], n_features=N))
        new = s.extract_orb(imgs[1], n_features=N)
        m, w_match = timed(lambda: s.match_descriptors([kp["desc"], new["desc"]]))
        both = float(np.median(w_ext)) + float(np.median(w_match))
        lines.append(f"ba_orb_extract of the second image, {N} features: wall {fmt(w_ext)}")
        lines.append(f"ba_match_descriptors, {len(kp['desc'])} x {len(new['desc'])}: wall {fmt(w_match)}; {int(m['n_good'][0])} good matches")
        lines.append(f"extract + match {both:.3f} ms; track {walls['defaults']:.3f} ms; ratio (extract + match) / track {both / walls['defaults']:.2f}")
        print("\n".join(lines[-3:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

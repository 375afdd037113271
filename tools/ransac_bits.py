"""Raw bits of ba_resect_ransac, ba_resect, ba_relative_pose, ba_homography, ba_sim3 and ba_fundamental (output of two builds side
by side in profiles/hypothesis_stage_bits.txt and profiles/ransac_stage_bits.txt).

    [BA_HIP_LIB=/other/build/libba_hip.so] python tools/ransac_bits.py [--out FILE] [--brief]

For the planted cases of tests/hypothesis_cases.py (seed 7) and the outlier cases of tests/test_gpu_ransac.py, test_gpu_relpose.py,
test_gpu_homography.py, test_gpu_sim3.py (with_scale 0 and 1) and test_gpu_fundamental.py (seed 0), and the edge pairs of
tests/fundamental_reference.py, with lo_rounds 0 and 2 and n_hyp 256 and 4096, pinhole and BAL for the resections (ba_resect: once
per problem): one line per output array with its SHA-256 (first 16 hex digits) and its first four 64-bit words (the bytes
themselves for narrower types); --brief: one line per call, the SHA-256 of all its output arrays in the order of their names
(what profiles/ransac_stage_bits.txt holds; without it the array that differs shows).  Two builds of the same ABI compute the same when their outputs are the same text; run each in a
process of its own."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = [(lo, n_hyp) for lo in (0, 2) for n_hyp in (256, 4096)]
PROBLEM_FIELDS = ("cams", "pts", "cam_idx", "pt_idx", "uv")


def build_inputs():
    """name -> array, "<call>/<case>/<field>": p1, p2, off, seed of a two-view case; the problem's fields and seed of a resection."""
    from tests import fundamental_reference as FD
    from tests import homography_reference as HG
    from tests import hypothesis_cases as HC
    from tests import ransac_reference as RS
    from tests import relpose_reference as RP
    from tests import sim3_reference as S3
    from tests.test_gpu_sim3 import SCENE_SEED
    d = {}

    def pairs(call, case, p1, p2, off, seed):
        off = np.array([0, len(p1)], dtype=np.int64) if off is None else off
        d.update({f"{call}/{case}/p1": p1, f"{call}/{case}/p2": p2, f"{call}/{case}/off": off, f"{call}/{case}/seed": np.int64(seed)})

    pairs("relpose", "planted", *HC.concatenated(HC.relpose_pairs()), HC.SEED)
    pairs("homography", "planted", *HC.concatenated(HC.plane_pairs()), HC.SEED)
    for share in (0.3, 0.5):
        for planar in (False, True):
            c = RP.outlier_case(planar, share)
            pairs("relpose", f"outliers planar={int(planar)} share={share}", c["p1"], c["p2"], None, 0)
        c = HG.outlier_case(share)
        pairs("homography", f"outliers share={share}", c["p1"], c["p2"], None, 0)
        for with_scale in (0, 1):
            c = S3.outlier_case(share, bool(with_scale), seed=SCENE_SEED)
            pairs("sim3", f"outliers share={share} with_scale={with_scale}", c["X1"], c["X2"], None, 0)
    for share, n_hyp, seed in FD.OUTLIER_CASES:
        c = FD.outlier_case(share, n_hyp, seed)
        pairs("fundamental", f"outliers share={share}", c["p1"], c["p2"], None, seed)
    edge = FD.edge_pairs()[0]
    pairs("fundamental", "edge pairs", np.concatenate([p[0] for p in edge]), np.concatenate([p[1] for p in edge]),
          np.r_[0, np.cumsum(FD.COUNTS)].astype(np.int64), 0)
    for model in HC.MODELS:
        probs = [("planted", HC.p3p_problem(model)["prob"], HC.SEED)] + [(f"outliers share={s}", RS.outlier_problem(model, s)[0], 0) for s in (0.3, 0.5)]
        for case, prob, seed in probs:
            d.update({f"resect {model}/{case}/{f}": getattr(prob, f) for f in PROBLEM_FIELDS})
            d[f"resect {model}/{case}/seed"] = np.int64(seed)
    d["K"], d["K4"], d["K sim3"] = HC.K, HC.K4, S3.K_TEST
    return d


def line(label, key, a):
    a = np.ascontiguousarray(a)
    raw = a.tobytes()
    head = " ".join(f"{w:016x}" for w in a.ravel()[:4].view(np.uint64)) if a.dtype.itemsize == 8 else raw[:16].hex()
    return f"{label} {key} {a.dtype}{list(a.shape)} sha256 {hashlib.sha256(raw).hexdigest()[:16]} head {head}"


def call_lines(label, out, brief):
    if not brief:
        return [line(label, k, out[k]) for k in sorted(out)]
    raw = b"".join(np.ascontiguousarray(out[k]).tobytes() for k in sorted(out))
    return [f"{label} {' '.join(sorted(out))} sha256 {hashlib.sha256(raw).hexdigest()[:32]}"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--brief", action="store_true")
    a = ap.parse_args()
    d = build_inputs()
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend as hb
    from bundle_adjustment_amd.bal import BALProblem
    from bundle_adjustment_amd.problem import BAProblem
    cases = sorted({k.rsplit("/", 1)[0] for k in d if "/" in k})
    lines = []
    with hb.Solver(0) as s:
        for case in cases:
            f = lambda name: d[f"{case}/{name}"]   # noqa: E731
            seed = int(f("seed"))
            if case.startswith("resect"):
                fields = [f(x) for x in PROBLEM_FIELDS]
                bal = fields[0].shape[1] == 9
                intr = s._set_bal(BALProblem(*fields).validate()) if bal else s.set_problem(BAProblem(*fields, d["K4"], 0).validate())
                out = s.resect(intr=intr)
                lines += call_lines(f"{case} ba_resect:", out, a.brief)
            for lo, n_hyp in SIZES:
                opts = dict(n_hyp=n_hyp, lo_rounds=lo, seed=seed)
                if case.startswith("resect"):
                    out = s.resect_ransac(intr=intr, **opts)
                elif case.startswith("sim3"):
                    out = s.sim3(d["K sim3"], f("p1"), f("p2"), f("off"), with_scale=int(case[-1]), **opts)
                elif case.startswith("fundamental"):
                    out = s.fundamental(f("p1"), f("p2"), f("off"), **opts)
                else:
                    call = s.relative_pose if case.startswith("relpose") else s.homography
                    out = call(d["K"], f("p1"), f("p2"), f("off"), **opts)
                lines += call_lines(f"{case} lo_rounds={lo} n_hyp={n_hyp}:", out, a.brief)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(text)


if __name__ == "__main__":
    main()

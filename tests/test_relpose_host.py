"""CPU: the yardstick of the relative-pose tests (tests/relpose_reference.py) against planted truth, and the surface of
ba_relative_pose that needs no device: the exported symbols, the options struct, the generator, estimate_pose's host side."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import relpose_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend.load_library()


def test_abi(lib):
    """The two symbols, the defaults, and struct ba_relpose_options of include/ba_hip.h: int32 x 2, uint64, double, int32 x 2,
    double x 2 = 48 bytes, no padding."""
    from bundle_adjustment_amd import hip_backend as hb
    assert hasattr(lib, "ba_relative_pose") and hasattr(lib, "ba_default_relpose_options")
    assert "ba_relative_pose" in hb.SYMBOLS and "ba_default_relpose_options" in hb.SYMBOLS
    o = hb.BARelposeOptions()
    assert lib.ba_default_relpose_options(C.byref(o)) == 0
    assert (o.n_hyp, o.lo_rounds, o.seed, o.max_epi_px, o.refine_iters, o.min_inliers, o.min_parallax_deg, o.max_depth) == \
        (256, 2, 0, 3.0, 20, 8, 0.0, 50.0)
    assert C.sizeof(hb.BARelposeOptions) == 48
    off = {k: getattr(hb.BARelposeOptions, k).offset for k, _ in hb.BARelposeOptions._fields_}
    assert off == dict(n_hyp=0, lo_rounds=4, seed=8, max_epi_px=16, refine_iters=24, min_inliers=28, min_parallax_deg=32, max_depth=40)
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"typedef struct ba_relpose_options \{(.*?)\} ba_relpose_options;", hdr, flags=re.S).group(1)
    names = re.findall(r"(?:int32_t|uint64_t|double)\s+([a-z_0-9]+)\s*;", body)
    assert names == [n for n, _ in hb.BARelposeOptions._fields_]
    enum = re.search(r"enum ba_relpose_status \{(.*?)\};", hdr, flags=re.S).group(1)
    codes = {k.lower(): int(v) for k, v in re.findall(r"BA_RELPOSE_([A-Z_]+) = (\d+)", enum)}
    assert codes == hb.RELPOSE_STATUS
    assert lib.ba_default_relpose_options(None) == -1 and b"null" in lib.ba_last_error()


def test_options_by_name():
    from bundle_adjustment_amd import hip_backend as hb

    class Lib:
        @staticmethod
        def ba_default_relpose_options(ref):
            ref._obj.n_hyp, ref._obj.lo_rounds = 256, 2
            return 0
    s = hb.Solver.__new__(hb.Solver)
    s._lib = Lib()
    o = s.relpose_options(n_hyp=64, seed=2 ** 63 + 5, max_depth=0.0)
    assert (o.n_hyp, o.seed, o.lo_rounds, o.max_depth) == (64, 2 ** 63 + 5, 2, 0.0)
    with pytest.raises(TypeError):
        s.relpose_options(no_such_option=1)


def test_generator():
    for n in (6, 7, 64, 1000):
        for h in range(300):
            i = R.sample5(7, 2, h, n)
            assert len(set(i)) == 5 and min(i) >= 0 and max(i) < n
            assert i == R.sample5(7, 2, h, n)
    assert len({R.sample5(0, 0, 0, 1000), R.sample5(1, 0, 0, 1000), R.sample5(0, 1, 0, 1000), R.sample5(0, 0, 1, 1000),
                R.sample5(0, 0, 0, 999)}) == 5
    # of n = 6 every index is drawn
    assert {x for h in range(64) for x in R.sample5(3, 0, h, 6)} == set(range(6))
    # pinned: (seed, pair, h, n)
    assert R.sample5(0, 0, 0, 1000) == (175, 473, 654, 137, 902)
    assert R.sample5(5, 3, 17, 64) == (32, 23, 62, 40, 51)
    assert R.sample5(2 ** 63 + 1, 65534, 4095, 7) == (5, 6, 1, 3, 4)


@pytest.mark.parametrize("planar", [False, True])
def test_reference_solver_finds_the_true_essential_matrix(planar):
    """200 noise-free samples of five matches (the planar scene an exact plane): the truth is among the solutions within 1e-6
    in every sample; every solution satisfies its five epipolar rows and the cubic constraints."""
    rng = np.random.default_rng(1)
    worst, worst_c, worst_e, nsol = 0.0, 0.0, 0.0, []
    for _ in range(200):
        p1, p2, Rm, t = R.make_scene(rng, 5, planar)
        x1, x2 = R.normalise(R.K_TEST, p1), R.normalise(R.K_TEST, p2)
        Es = R.five_point(x1, x2)
        nsol.append(len(Es))
        assert Es
        worst = max(worst, min(R.E_distance(E, R.essential(Rm, t)) for E in Es))
        for E in Es:
            h1, h2 = np.c_[x1, np.ones(5)], np.c_[x2, np.ones(5)]
            worst_e = max(worst_e, float(np.abs(((h2 @ E) * h1).sum(1)).max()))
            worst_c = max(worst_c, *R.cubic_residual(E))
    print(f"planar={planar}: worst distance to the truth {worst:.2e}; epipolar rows {worst_e:.2e}; cubics {worst_c:.2e}; "
          f"{np.mean(nsol):.2f} solutions on average, {max(nsol)} at most")
    assert worst <= 1e-6
    assert worst_e <= 1e-6 and worst_c <= 1e-6 and max(nsol) <= 10      # (the bound on E itself)


@pytest.mark.parametrize("planar", [False, True])
@pytest.mark.parametrize("share", [0.3, 0.5])
def test_reference_ransac_recovers_the_planted_inliers(planar, share):
    c = R.outlier_case(planar, share)
    ref = c["ref"]
    print(f"planar={planar} share={share}: reference against the yardstick: rotation {c['d_ref'][0]:.2e} rad, translation direction "
          f"{c['d_ref'][1]:.2e} rad; against the truth {R.pose_distance(ref['R'], ref['t'], c['R'], c['t'])}")
    assert ref["status"] == R.OK
    assert np.array_equal(ref["match_inlier"], ~c["planted"]) and ref["n_inliers"] == (~c["planted"]).sum()
    assert max(c["d_ref"]) <= 1e-12
    assert ref["rms_px"] < 0.6 and ref["parallax_deg"] > 5.0


class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


class _FakeSolver:
    """hip_backend.Solver.relative_pose answered by the numpy reference."""

    def __init__(self, **force):
        self.force, self.seen = force, None

    def relative_pose(self, K, pts1, pts2, pair_off=None, **opts):
        self.seen = (np.asarray(pts1), np.asarray(pts2), opts)
        r = R.relative_pose(K, np.asarray(pts1, dtype=np.float64), np.asarray(pts2, dtype=np.float64), **opts)
        r.update(self.force)
        return dict(R=r["R"][None], t=r["t"][None], status=np.array([r["status"]], dtype=np.uint8),
                    n_inliers=np.array([r["n_inliers"]], dtype=np.int32), rms_px=np.array([r["rms_px"]]),
                    parallax_deg=np.array([r["parallax_deg"]]), best_hyp=np.array([r["best_hyp"]], dtype=np.int32),
                    match_inlier=r["match_inlier"])


def test_estimate_pose_host_side(capsys):
    from bundle_adjustment_amd import estimate_pose, relative_pose  # noqa: F401  (exported from the package)
    c = R.outlier_case(False, 0.5)
    n = len(c["p1"])
    perm = np.random.default_rng(0).permutation(n)
    kp1 = [_KeyPoint(p) for p in c["p1"]]
    kp2 = [None] * n
    for i, j in enumerate(perm):
        kp2[j] = _KeyPoint(c["p2"][i])
    matches = [_Match(i, int(perm[i])) for i in range(n)]
    fake = _FakeSolver()
    Rr, tr, i1, i2, idx = estimate_pose(matches, kp1, kp2, R.K_TEST, solver=fake, n_hyp=64)
    out = capsys.readouterr().out.splitlines()
    assert fake.seen[0].dtype == np.float32 and fake.seen[2] == dict(n_hyp=64)
    assert Rr.shape == (3, 3) and tr.shape == (3, 1) and Rr.dtype == tr.dtype == np.float64
    assert i1.dtype == i2.dtype == np.float32 and i1.shape == i2.shape == (len(idx), 2)
    assert np.array_equal(idx, np.nonzero(~c["planted"])[0])
    assert np.array_equal(i1, np.float32(c["p1"])[idx]) and np.array_equal(i2, np.float32(c["p2"])[idx])
    assert out == [f"    -> Pose Estimation: {len(idx)} inliers out of {n} matches (Ratio: {len(idx) / n:.2f})"]
    assert max(R.pose_distance(Rr, tr.ravel(), c["R"], c["t"])) < 0.02
    # a low ratio prints the reference's warning; quiet prints nothing
    low = _FakeSolver(match_inlier=np.arange(n) < 30)
    estimate_pose(matches, kp1, kp2, R.K_TEST, solver=low, n_hyp=8)
    out = capsys.readouterr().out.splitlines()
    assert out == [f"    -> Pose Estimation: 30 inliers out of {n} matches (Ratio: 0.10)",
                   "    -> WARNING: Low inlier ratio. Pose estimate may be unreliable."]
    estimate_pose(matches, kp1, kp2, R.K_TEST, solver=low, quiet=True, n_hyp=8)
    assert capsys.readouterr().out == ""
    # no pose: five None
    assert estimate_pose(matches[:5], kp1, kp2, R.K_TEST, solver=_FakeSolver()) == (None,) * 5
    assert estimate_pose(matches, kp1, kp2, R.K_TEST, solver=_FakeSolver(status=R.DEGENERATE, best_hyp=-1), n_hyp=1) == (None,) * 5
    got = estimate_pose(matches, kp1, kp2, R.K_TEST, solver=_FakeSolver(status=R.FEW_INLIERS), quiet=True, n_hyp=8)
    assert got[0] is not None

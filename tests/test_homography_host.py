"""CPU: the yardstick of the homography tests (tests/homography_reference.py) against planted truth, and the surface of
ba_homography that needs no device: the exported symbols, the options struct, the generator, the margins that entitle
tests/test_gpu_homography.py to demand the planted inlier set exactly, and estimate_two_view's selection on stubbed outputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import homography_reference as H
from tests import relpose_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = H.K_TEST
DRAWS = range(12)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend.load_library()


def test_abi(lib):
    """The two symbols, the defaults, and struct ba_homography_options of include/ba_hip.h: int32 x 2, uint64, double, int32 x 2,
    double x 3 = 56 bytes, no padding."""
    from bundle_adjustment_amd import hip_backend as hb
    assert hasattr(lib, "ba_homography") and hasattr(lib, "ba_default_homography_options")
    assert "ba_homography" in hb.SYMBOLS and "ba_default_homography_options" in hb.SYMBOLS
    o = hb.BAHomographyOptions()
    assert lib.ba_default_homography_options(C.byref(o)) == 0
    assert (o.n_hyp, o.lo_rounds, o.seed, o.max_px, o.refine_iters, o.min_inliers, o.max_depth, o.ambiguity_ratio, o.min_translation) == \
        (256, 2, 0, 3.0, 20, 8, 50.0, 0.75, H.MIN_TRANSLATION)
    assert C.sizeof(hb.BAHomographyOptions) == 56
    off = {k: getattr(hb.BAHomographyOptions, k).offset for k, _ in hb.BAHomographyOptions._fields_}
    assert off == dict(n_hyp=0, lo_rounds=4, seed=8, max_px=16, refine_iters=24, min_inliers=28, max_depth=32, ambiguity_ratio=40,
                       min_translation=48)
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"typedef struct ba_homography_options \{(.*?)\} ba_homography_options;", hdr, flags=re.S).group(1)
    names = re.findall(r"(?:int32_t|uint64_t|double)\s+([a-z_0-9]+)\s*;", body)
    assert names == [n for n, _ in hb.BAHomographyOptions._fields_]
    enum = re.search(r"enum ba_homography_status \{(.*?)\};", hdr, flags=re.S).group(1)
    codes = {k.lower(): int(v) for k, v in re.findall(r"BA_HOMOGRAPHY_([A-Z_]+) = (\d+)", enum)}
    assert codes == hb.HOMOGRAPHY_STATUS
    assert [codes[k] for k in ("ok", "few_matches", "degenerate", "few_inliers", "rotation", "ambiguous")] == \
        [H.OK, H.FEW_MATCHES, H.DEGENERATE, H.FEW_INLIERS, H.ROTATION, H.AMBIGUOUS]
    assert lib.ba_default_homography_options(None) == -1 and b"null" in lib.ba_last_error()


def test_options_by_name():
    from bundle_adjustment_amd import hip_backend as hb

    class Lib:
        @staticmethod
        def ba_default_homography_options(ref):
            ref._obj.n_hyp, ref._obj.lo_rounds, ref._obj.ambiguity_ratio = 256, 2, 0.75
            return 0
    s = hb.Solver.__new__(hb.Solver)
    s._lib = Lib()
    o = s.homography_options(n_hyp=64, seed=2 ** 63 + 5, max_px=1.5, min_translation=0.1)
    assert (o.n_hyp, o.seed, o.lo_rounds, o.max_px, o.ambiguity_ratio, o.min_translation) == (64, 2 ** 63 + 5, 2, 1.5, 0.75, 0.1)
    with pytest.raises(TypeError):
        s.homography_options(max_epi_px=1.0)


def test_generator():
    """Four distinct indices; the draws d = 0 .. 3 are those of ba_relative_pose's generator, whose pinned values
    (tests/test_relpose_host.py) were computed by hand."""
    for n in (4, 5, 64, 1000):
        for h in range(300):
            i = H.sample4(7, 2, h, n)
            assert len(set(i)) == 4 and min(i) >= 0 and max(i) < n
            assert i == H.sample4(7, 2, h, n)
            if n >= 5:
                assert i == R.sample5(7, 2, h, n)[:4]
    assert len({H.sample4(0, 0, 0, 1000), H.sample4(1, 0, 0, 1000), H.sample4(0, 1, 0, 1000), H.sample4(0, 0, 1, 1000),
                H.sample4(0, 0, 0, 500)}) == 5
    assert {x for h in range(64) for x in H.sample4(3, 0, h, 5)} == set(range(5))
    # pinned: (seed, pair, h, n)
    assert H.sample4(0, 0, 0, 1000) == (175, 473, 654, 137)
    assert H.sample4(5, 3, 17, 64) == (32, 23, 62, 40)
    assert H.sample4(2 ** 63 + 1, 65534, 4095, 7) == (5, 6, 1, 3)


def test_closed_form_against_the_dlt_null_vector():
    """240 noise-free samples of four matches on the exact plane: the closed form of step 3 and the null vector of the 8 x 9
    DLT (LAPACK's SVD) both reproduce the plane's true homography.  1e-9 is the bound on a unit-norm H~ in fp64 at these
    samples' conditioning; measured: 8.8e-12 (closed form) and 1.3e-11 (DLT)."""
    rng = np.random.default_rng(0)
    worst, worst_dlt, between, void = 0.0, 0.0, 0.0, 0
    for s in range(60):
        p1, p2, _, _, Ht = H.plane_scene(rng, 8)
        x1, x2 = R.normalise(K, p1), R.normalise(K, p2)
        for seed in range(4):
            idx = list(H.sample4(seed, s, 0, 8))
            Hc = H.four_point(x1[idx], x2[idx])
            if Hc is None:
                void += 1
                continue
            Hd = H.four_point_dlt(x1[idx], x2[idx])
            worst, worst_dlt = max(worst, H.H_distance(Hc, Ht)), max(worst_dlt, H.H_distance(Hd, Ht))
            between = max(between, H.H_distance(Hc, Hd))
            assert abs(np.linalg.norm(Hc) - 1.0) <= 1e-15 and np.linalg.det(Hc) > 0.0
    print(f"closed form against the truth {worst:.2e}, DLT null vector {worst_dlt:.2e}, between the two {between:.2e}; {void} void of 240")
    assert worst <= 1e-9 and worst_dlt <= 1e-9 and void <= 2


def test_void_samples():
    sq = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    assert H.four_point(sq, sq + 0.5) is not None
    line = np.array([[0.0, 0.0], [0.5, 0.5], [1.0, 1.0], [0.0, 1.0]])
    assert H.four_point(line, sq) is None and H.four_point(sq, line) is None          # a collinear triple in either image
    twice = np.array([[0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    assert H.four_point(twice, sq) is None
    bow = sq[[0, 2, 1, 3]]                                                             # a twisted quadrilateral: no orientation-preserving H
    assert H.four_point(sq, bow) is None


def test_refinement_rejects_a_trial_that_puts_a_match_behind_a_camera():
    """Step 5: such an H~ costs infinity, so the refinement never trades a match for a lower cost.  Started (against the header,
    whose start is a consensus set) at an H~ whose third row turns one match's third component negative, the infinite first cost
    is undercut only by a trial with every match in front, and the refinement ends at one."""
    p1, p2, _, _, Ht = H.noisy_plane(0, 40)
    x1, x2 = R.normalise(K, p1), R.normalise(K, p2)
    assert H.residual_jacobian(Ht, x1, x2)[2]
    far = int(np.argmax(x1[:, 0]))
    bad = Ht.copy()
    bad[2] = [-Ht[2, 2] / x1[far, 0] * 1.01, 0.0, Ht[2, 2]]          # (H~ x1~)_2 < 0 at the right-most match only
    bad = H.unit_H(bad)
    r, J, front = H.residual_jacobian(bad, x1, x2)
    assert not front and len(r) < 4 * 40
    got, ok = H.refine(bad, x1, x2)
    assert ok and not np.array_equal(got, bad) and H.residual_jacobian(got, x1, x2)[2]
    got, ok = H.refine(Ht, x1, x2)
    assert ok and H.residual_jacobian(got, x1, x2)[2] and H.H_distance(got, Ht) < 1e-2


def test_every_candidate_reproduces_the_homography_and_the_truth_is_among_them():
    worst, found = 0.0, 0
    for seed in DRAWS:
        _, _, Rt, tt, Ht = H.noisy_plane(seed)
        d2 = H.singular_values(Ht)[1]
        n_true = H.true_plane_pose(Rt, tt)[2]
        hit = False
        cands = H.candidates(Ht)
        assert len(cands) == 4
        for Rc, tc, nc, s in cands:
            worst = max(worst, float(np.abs(Ht / d2 - (Rc + s * np.outer(tc, nc))).max()))
            assert abs(np.linalg.det(Rc) - 1.0) <= 1e-12 and abs(np.linalg.norm(tc) - 1.0) <= 1e-12 and abs(np.linalg.norm(nc) - 1.0) <= 1e-12
            hit |= max(R.pose_distance(Rc, tc, Rt, tt)) <= 1e-9 and np.abs(nc - n_true).max() <= 1e-9
        assert np.array_equal(cands[0][0], cands[1][0]) and np.array_equal(cands[0][1], -cands[1][1]) and np.array_equal(cands[0][2], -cands[1][2])
        found += hit
        # |t| / d of the scene: the baseline over the plane's distance
        assert abs(cands[0][3] - R.BASELINE * np.linalg.norm(H.PLANE_N) / H.PLANE_D) <= 1e-12
    print(f"worst |H~ / d2 - (R + (t / d) n^T)| over 48 candidates {worst:.2e}; the truth is among them in {found} of 12 draws")
    assert worst <= 1e-14 and found == 12


def test_votes_on_the_noise_free_plane():
    """The truth gets every vote, the candidate with t and n flipped none; in some draws the second pose gets every vote too."""
    full = []
    for seed in DRAWS:
        rng = np.random.default_rng(seed)
        p1, p2, Rt, tt, Ht = H.plane_scene(rng, 300)
        x1, x2 = R.normalise(K, p1), R.normalise(K, p2)
        inl = np.ones(300, dtype=bool)
        dec = H.decompose(Ht, x1, x2, inl, 3.0 / 805.0, 50.0, H.MIN_TRANSLATION, 0.75)
        assert dec["votes"][0] == 300 and dec["n_pose"] >= 1 and not dec["rotation"]
        d = [max(R.pose_distance(dec["R"][k], dec["t"][k], Rt, tt)) for k in range(2)]
        assert min(d) <= 1e-9
        if d[0] > 1e-9:
            assert dec["ambiguous"] and dec["votes"][1] == 300
        full.append(int(dec["votes"][1]) == 300)
        for Rc, tc, nc, _ in H.candidates(Ht):
            if max(R.pose_distance(Rc, -tc, Rt, tt)) <= 1e-9:       # the truth's flipped twin
                front, _ = R.in_front(Rc, tc, x1, x2, 50.0)
                assert not (front & (H.hom(x1) @ nc > 0.0)).any()
    print(f"second pose with 300 of 300 votes in draws {[s for s, f in zip(DRAWS, full) if f]}")
    assert sum(full) >= 1


def test_min_translation_default_lies_between_rotation_and_plane():
    """ba_homography_options.min_translation: (d1 - d3) / d2 of the refined H~ under a pure rotation with 0.3 px of noise (12 draws)
    against the tests' plane at its 17 degrees of parallax, noise-free (the ratio is |t| / d, 0.3629 in every draw).  The default is
    the geometric mean of the largest of the first and the smallest of the second, to two digits."""
    rot, plane = [], []
    for seed in DRAWS:
        p1, p2, _ = H.rotation_scene(seed)
        r = H.homography(K, p1, p2, n_hyp=64, min_translation=0.0)
        assert r["n_inliers"] == 300
        d = H.singular_values(r["Hn"])
        rot.append((d[0] - d[2]) / d[1])
        d = H.singular_values(H.noisy_plane(seed)[4])
        plane.append((d[0] - d[2]) / d[1])
    gm = float(np.sqrt(max(rot) * min(plane)))
    print(f"pure rotation {min(rot):.2e} .. {max(rot):.2e}; plane {min(plane):.4f} .. {max(plane):.4f}; geometric mean {gm:.4f}")
    assert max(rot) < H.MIN_TRANSLATION < min(plane)
    assert abs(gm - H.MIN_TRANSLATION) <= 0.0005


@pytest.mark.parametrize("share", [0.3, 0.5])
def test_outlier_margins_and_the_reference_ransac(share):
    """At the yardstick every true match errs below 0.8 thr and every planted mismatch above 1.25 thr (the larger of the two
    transfer errors): the condition under which "the planted set exactly" is a fair demand.  The reference's own RANSAC
    recovers the planted set and reaches the yardstick."""
    c = H.outlier_case(share)
    x1, x2 = R.normalise(K, c["p1"]), R.normalise(K, c["p2"])
    thr = 3.0 / (0.5 * (K[0, 0] + K[1, 1]))
    f, b, pf, pb = H.transfer(c["yard"], x1, x2)
    with np.errstate(invalid="ignore"):
        e = np.where(pf & pb, np.sqrt(np.maximum(f, b)), np.inf)
    pl = c["planted"]
    print(f"share={share}: true matches err up to {e[~pl].max() / thr:.3f} thr, planted mismatches from {e[pl].min() / thr:.2f} thr; "
          f"reference to the yardstick {c['d_ref']:.2e}, to the truth {H.H_distance(c['ref']['Hn'], c['Ht']):.2e}")
    assert pl.sum() == round(share * 300)
    assert e[~pl].max() < 0.8 * thr and e[pl].min() > 1.25 * thr
    ref = c["ref"]
    assert ref["status"] == H.OK
    assert np.array_equal(ref["match_inlier"], ~pl) and ref["n_inliers"] == (~pl).sum()
    assert c["d_ref"] <= 1e-12
    assert ref["rms_px"] < 0.7 and H.H_distance(ref["H"], H.pixel_H(K, ref["Hn"])) == 0.0
    assert max(R.pose_distance(ref["R"][0], ref["t"][0], c["R"], c["t"])) < 0.02


# ------------------------------------------------------------------------------------------------------------ estimate_two_view
class _Match:
    def __init__(self, q, t):
        self.queryIdx, self.trainIdx = q, t


class _KeyPoint:
    def __init__(self, pt):
        self.pt = (float(pt[0]), float(pt[1]))


class _Stub:
    """hip_backend.Solver's two calls answered by fixed outputs for n matches."""

    def __init__(self, n, e_inl, h_inl, h_status=0, e_status=0, votes=(90, 10), n_pose=2, h_best=0, e_best=0):
        self.n, self.calls = n, []
        self.e = dict(R=np.eye(3)[None] * 1.0, t=np.array([[1.0, 0.0, 0.0]]), status=np.array([e_status], dtype=np.uint8),
                      n_inliers=np.array([e_inl], dtype=np.int32), rms_px=np.array([0.5]), parallax_deg=np.array([10.0]),
                      best_hyp=np.array([e_best], dtype=np.int32), match_inlier=np.arange(n) < e_inl)
        Rh = np.stack([R.exp_so3(np.array([0.0, 0.1, 0.0])), R.exp_so3(np.array([0.0, 0.2, 0.0]))])[None]
        self.h = dict(H=np.eye(3)[None], status=np.array([h_status], dtype=np.uint8), n_inliers=np.array([h_inl], dtype=np.int32),
                      rms_px=np.array([0.5]), best_hyp=np.array([h_best], dtype=np.int32), n_pose=np.array([n_pose], dtype=np.int32),
                      match_inlier=np.arange(n) >= n - h_inl, R=Rh, t=np.array([[[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]]),
                      normal=np.array([[[0.0, 0.0, 1.0], [0.0, 0.6, 0.8]]]), t_over_d=np.full((1, 2), 0.3),
                      votes=np.array([votes], dtype=np.int32), pose_cost=np.zeros((1, 2)))

    def relative_pose(self, K, pts1, pts2, pair_off=None, **opts):
        self.calls.append(("E", opts))
        return self.e

    def homography(self, K, pts1, pts2, pair_off=None, **opts):
        self.calls.append(("H", opts))
        return self.h


def test_estimate_two_view_selection(capsys):
    from bundle_adjustment_amd import estimate_pose, estimate_two_view, homography  # noqa: F401  (exported from the package)
    n = 100
    kp = [_KeyPoint((10.0 * i, 5.0 * i)) for i in range(n)]
    matches = [_Match(i, i) for i in range(n)]

    def run(stub, **kw):
        return estimate_two_view(matches, kp, kp, K, solver=stub, **kw)

    # the homography explains as many matches as the essential matrix: its first pose, its inliers
    s = _Stub(n, e_inl=90, h_inl=80)
    Rr, tr, i1, i2, idx, info = run(s, n_hyp=32, max_px=2.0, max_epi_px=1.0)
    assert info["model"] == "homography" and np.array_equal(Rr, s.h["R"][0, 0]) and np.array_equal(tr.ravel(), [0.0, 1.0, 0.0])
    assert tr.shape == (3, 1) and np.array_equal(idx, np.arange(20, 100)) and i1.dtype == np.float32 and len(i1) == len(i2) == 80
    assert np.array_equal(info["normal"], [0.0, 0.0, 1.0]) and np.array_equal(info["second_pose"][0], s.h["R"][0, 1])
    assert info["second_pose"][1].shape == (3, 1) and np.array_equal(info["second_pose"][2], [0.0, 0.6, 0.8])
    assert s.calls == [("E", dict(n_hyp=32, max_epi_px=1.0)), ("H", dict(n_hyp=32, max_px=2.0))]
    assert info["essential"]["n_inliers"] == 90 and info["homography"]["n_inliers"] == 80
    out = capsys.readouterr().out.splitlines()
    assert out == ["    -> Two-view model: homography (80 homography inliers, 90 essential)",
                   f"    -> Pose Estimation: 80 inliers out of {n} matches (Ratio: 0.80)"]
    # below the ratio: the essential pose, estimate_pose's values bit for bit
    s = _Stub(n, e_inl=90, h_inl=71)
    got = run(s)
    want = estimate_pose(matches, kp, kp, K, solver=s)
    assert got[5]["model"] == "essential" and got[5]["second_pose"] is None and got[5]["normal"] is None
    for a, b in zip(got[:5], want):
        assert np.array_equal(a, b) and a.dtype == b.dtype
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == lines[1] == f"    -> Pose Estimation: 90 inliers out of {n} matches (Ratio: 0.90)"
    assert run(_Stub(n, e_inl=90, h_inl=72), quiet=True)[5]["model"] == "homography"      # 72 >= 0.8 * 90
    assert run(_Stub(n, e_inl=90, h_inl=72), quiet=True, planar_ratio=0.9)[5]["model"] == "essential"
    assert capsys.readouterr().out == ""
    # the homography's status decides the rest
    Rr, tr, i1, i2, idx, info = run(_Stub(n, 90, 88, h_status=H.ROTATION, n_pose=1, votes=(0, 0)), quiet=True)
    assert info["model"] == "rotation" and Rr.shape == (3, 3) and len(i1) == len(i2) == len(idx) == 0 and info["second_pose"] is None
    Rr, tr, i1, i2, idx, info = run(_Stub(n, 90, 88, h_status=H.AMBIGUOUS, votes=(88, 80)), quiet=True)
    assert info["model"] == "ambiguous" and len(idx) == 0 and info["second_pose"] is not None and Rr is not None
    for bad in (H.FEW_INLIERS, H.DEGENERATE):
        assert run(_Stub(n, 90, 88, h_status=bad), quiet=True)[5]["model"] == "essential"
    assert run(_Stub(n, 90, 0, h_status=H.DEGENERATE, h_best=-1), quiet=True)[5]["model"] == "essential"
    assert run(_Stub(n, 0, 0, h_status=H.DEGENERATE, h_best=-1, e_status=R.FEW_INLIERS), quiet=True)[5]["model"] == "essential"
    assert run(_Stub(n, 90, 88, votes=(50, 50)), quiet=True)[5]["model"] == "essential"     # ok, but no pose carries the most votes
    # no pose at all: five None and the dict
    got = run(_Stub(n, 0, 0, h_status=H.FEW_MATCHES, h_best=-1, e_status=R.FEW_MATCHES, e_best=-1), quiet=True)
    assert got[:5] == (None,) * 5 and got[5]["model"] == "essential"
    with pytest.raises(TypeError):
        run(_Stub(n, 90, 80), no_such_option=1)


def test_match_by_homography_host_side():
    """The window handed to Solver.match_guided: pi(H kp1) and the radius; -1 where the prediction does not exist."""
    from bundle_adjustment_amd import match_by_homography
    seen = {}

    class Guided:
        def match_guided(self, sets, kps, window=None, **opts):
            seen.update(sets=sets, kps=kps, window=window, opts=opts)
            n = len(sets[0])
            return dict(row_off=np.array([0, n]), good=np.ones(n, dtype=bool), best=np.arange(n, dtype=np.int32), dist1=np.zeros(n, dtype=np.int32))

    Hm = np.array([[1.0, 0.0, 10.0], [0.0, 1.0, -5.0], [0.001, 0.0, 1.0]])
    kp1 = np.array([[100.0, 50.0], [0.0, 0.0], [-2000.0, 10.0]])                        # the third: third component -1
    des = np.zeros((3, 32), dtype=np.uint8)
    q, t, d = match_by_homography(des, kp1, des, [_KeyPoint(p) for p in kp1], Hm, 7.5, solver=Guided(), ratio=0.9)
    assert np.array_equal(q, [0, 1, 2]) and seen["opts"] == dict(ratio=0.9)
    w = seen["window"]
    assert w.dtype == np.float32 and w.shape == (3, 3)
    assert np.allclose(w[0], [110.0 / 1.1, 45.0 / 1.1, 7.5]) and np.allclose(w[1], [10.0, -5.0, 7.5]) and np.array_equal(w[2], [0.0, 0.0, -1.0])
    assert np.array_equal(seen["kps"][0], kp1) and np.array_equal(seen["kps"][1], kp1)
    assert all(len(x) == 0 for x in match_by_homography(None, kp1, des, kp1, Hm, 5.0, solver=Guided()))

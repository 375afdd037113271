"""CPU: the yardstick of the KLT tests (tests/klt_reference.py) against ground truth on an analytic image, its statuses on small
inputs, its weights at the ties, and the surface of ba_track_klt that needs no device: the level function, the options struct,
the refusals of the options, features.py's argument checks."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import klt_reference as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend.load_library()


# (H, W, half_window, max_level) -> (level_w, level_h)
LEVEL_CASES = [
    (21, 21, 10, 3, [21], [21]),                                # the smallest legal image: one level
    (41, 41, 10, 3, [41, 21], [41, 21]),                        # (41 + 1) / 2 = 21 >= 21 binds on both sides
    (43, 42, 10, 3, [42, 21], [43, 22]),                        # ... and on the width alone
    (150, 200, 10, 3, [200, 100, 50], [150, 75, 38]),           # 25 x 19 would be below the window
    (150, 200, 10, 1, [200, 100], [150, 75]),                   # max_level binds
    (480, 640, 1, 8, [640, 320, 160, 80, 40, 20, 10, 5], [480, 240, 120, 60, 30, 15, 8, 4]),       # 3 x 2 is below 3 x 3
    (800, 1000, 1, 8, [1000, 500, 250, 125, 63, 32, 16, 8, 4], [800, 400, 200, 100, 50, 25, 13, 7, 4]),
]


@pytest.mark.parametrize("H,W,hw,ml,lw,lh", LEVEL_CASES)
def test_levels_equal_the_reference(lib, H, W, hw, ml, lw, lh):
    from bundle_adjustment_amd import hip_backend as hb
    gw, gh = hb.klt_levels(H, W, half_window=hw, max_level=ml)
    rw, rh = K.levels(H, W, half_window=hw, max_level=ml)
    assert gw.dtype == np.int32 and gw.tolist() == rw.tolist() == lw and gh.tolist() == rh.tolist() == lh


def test_abi_and_refusals_without_a_device(lib):
    from bundle_adjustment_amd import hip_backend as hb
    for name in ("ba_default_klt_options", "ba_klt_levels", "ba_track_klt"):
        assert hasattr(lib, name) and name in hb.SYMBOLS
    o = hb.BAKltOptions()
    assert lib.ba_default_klt_options(C.byref(o)) == 0
    assert (o.half_window, o.max_level, o.max_iters, o.reserved, o.eps, o.min_eig, o.fb_max_px) == (10, 3, 30, 0, 0.01, 1e-4, 0.0)
    assert C.sizeof(hb.BAKltOptions) == 40
    off = {k: getattr(hb.BAKltOptions, k).offset for k, _ in hb.BAKltOptions._fields_}
    assert off == dict(half_window=0, max_level=4, max_iters=8, reserved=12, eps=16, min_eig=24, fb_max_px=32)
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"typedef struct ba_klt_options \{(.*?)\} ba_klt_options;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(hb.BAKltOptions._fields_)
    enum = re.search(r"enum ba_klt_status \{(.*?)\};", hdr).group(1)
    assert {k.lower(): int(v) for k, v in re.findall(r"BA_KLT_([A-Z_]+) = (\d)", enum)} == hb.KLT_STATUS
    assert (K.OK, K.OUT, K.FLAT, K.FB_FAIL) == tuple(hb.KLT_STATUS[k] for k in ("ok", "out", "flat", "fb_fail"))
    src = open(os.path.join(ROOT, "bundle_adjustment_amd", "csrc", "ba_klt.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (KLT_[A-Z_]+) = (\d+);", src)}
    assert (consts["KLT_TILE_W"], consts["KLT_TILE_H"], consts["KLT_MAX_LEVELS"], consts["KLT_MAX_HALF"]) == \
        (hb.KLT_TILE_W, hb.KLT_TILE_H, hb.KLT_MAX_LEVELS, hb.KLT_MAX_HALF)
    assert lib.ba_default_klt_options(None) == -1 and b"null" in lib.ba_last_error()
    assert lib.ba_klt_levels(None, 100, 100, None, None, None) == -1 and b"null" in lib.ba_last_error()
    assert lib.ba_klt_levels(C.byref(o), 100, 100, None, None, None) == 0              # every output may be NULL
    assert lib.ba_track_klt(None, 0, 100, 100, None, 0, None, None, None, None, C.byref(o), None, None, None, None) == -1
    with pytest.raises(TypeError):
        hb.klt_options(win_size=21)
    nan = float("nan")
    for kw, field in ((dict(half_window=0), "half_window"), (dict(half_window=16), "half_window"), (dict(max_level=-1), "max_level"),
                      (dict(max_level=9), "max_level"), (dict(max_iters=0), "max_iters"), (dict(max_iters=101), "max_iters"),
                      (dict(eps=-1e-9), "eps"), (dict(eps=nan), "eps"), (dict(min_eig=-1.0), "min_eig"), (dict(min_eig=nan), "min_eig"),
                      (dict(fb_max_px=nan), "fb_max_px")):
        with pytest.raises(hb.BAHipError, match=field):
            hb.klt_levels(100, 100, **kw)
    for H, W, field in ((0, 100, "height"), (100, -1, "width"), (20, 100, "window"), (100, 20, "window")):
        with pytest.raises(hb.BAHipError, match=field):
            hb.klt_levels(H, W)
    assert len(hb.klt_levels(21, 21)[0]) == 1 and len(hb.klt_levels(31, 31, half_window=15)[0]) == 1
    hb.klt_levels(100, 100, eps=0.0, min_eig=0.0, fb_max_px=-1.0, half_window=15, max_level=8, max_iters=100)      # the ranges' ends


def test_weights():
    assert K.weights(0.0, 0.0) == (16384, 0, 0, 0)
    assert K.weights(0.5, 0.5) == (4096, 4096, 4096, 4096)
    assert K.weights(0.5, 0.0) == (8192, 8192, 0, 0) and K.weights(0.0, 0.5) == (8192, 0, 8192, 0)
    # (1 - 2^-15) * 16384 = 16383.5 is a tie and goes to the even 16384; 2^-15 * 16384 = 0.5 goes to 0
    assert (1.0 - 2.0 ** -15) * 16384.0 == 16383.5
    assert K.weights(2.0 ** -15, 0.0) == (16384, 0, 0, 0) and K.weights(0.0, 2.0 ** -15) == (16384, 0, 0, 0)
    assert K.weights(3 * 2.0 ** -15, 0.0) == (16382, 2, 0, 0)            # 16382.5 -> 16382, 1.5 -> 2
    # 16382.8 -> 16383 and twice 0.6 -> 1: the three rounded weights exceed 16384 and w11 takes the difference, as the formula says
    assert K.weights(1.2 * 2.0 ** -15, 1.2 * 2.0 ** -15) == (16383, 1, 1, -1)
    rng = np.random.default_rng(0)
    for a, b in np.r_[rng.uniform(0, 1, (4000, 2)), rng.integers(0, 1 << 15, (4000, 2)) / float(1 << 15)]:
        w = K.weights(a, b)
        assert sum(w) == 16384 and min(w[:3]) >= 0 and -1 <= w[3] <= 16384
    # a constant array samples to the constant, whatever the weights
    A = np.full((30, 30), 200, dtype=np.int64)
    assert (K.sample(A, 3.3, 4.7, 7, 9) == 200 * 32).all() and (K.sample(-A, 3.3, 4.7, 7, 14) == -200).all()
    # the sample against a literal loop, window partly outside the image
    A = rng.integers(-4080, 4081, (9, 11))
    got = K.sample(A, -1.25, 5.5, 5, 14)
    w00, w01, w10, w11 = K.weights(0.75, 0.5)
    for i in range(5):
        for j in range(5):
            at = lambda x, y: int(A[min(max(y, 0), 8), min(max(x, 0), 10)])
            v = w00 * at(-2 + j, 5 + i) + w01 * at(-1 + j, 5 + i) + w10 * at(-2 + j, 6 + i) + w11 * at(-1 + j, 6 + i) + 8192
            assert int(got[i, j]) == v >> 14


def test_pyramid_and_gradients_against_loops():
    rng = np.random.default_rng(3)
    P = rng.integers(0, 256, (9, 12)).astype(np.uint8)
    D = K.down(P)
    assert D.shape == (5, 6)
    g = [1, 4, 6, 4, 1]
    refl = lambda i, n: (-i if i < 0 else 2 * n - 2 - i if i >= n else i)
    for y in range(5):
        for x in range(6):
            s = sum(g[i + 2] * g[j + 2] * int(P[refl(2 * y + i, 9), refl(2 * x + j, 12)]) for i in range(-2, 3) for j in range(-2, 3))
            assert int(D[y, x]) == (s + 128) >> 8
    assert [refl(i, 9) for i in (-2, -1, 9, 10)] == [2, 1, 7, 6]
    Ix, Iy = K.scharr(P)
    at = lambda x, y: int(P[min(max(y, 0), 8), min(max(x, 0), 11)])
    for y in range(9):
        for x in range(12):
            assert int(Ix[y, x]) == 3 * (at(x + 1, y - 1) - at(x - 1, y - 1)) + 10 * (at(x + 1, y) - at(x - 1, y)) + 3 * (at(x + 1, y + 1) - at(x - 1, y + 1))
            assert int(Iy[y, x]) == 3 * (at(x - 1, y + 1) - at(x - 1, y - 1)) + 10 * (at(x, y + 1) - at(x, y - 1)) + 3 * (at(x + 1, y + 1) - at(x + 1, y - 1))
    assert (K.down(np.full((40, 30), 77, np.uint8)) == 77).all() and np.abs(Ix).max() <= 16 * 255


SHIFTS = [(0.37, -0.21), (3.3, 2.6), (11.7, -9.4)]


@pytest.fixture(scope="module")
def analytic():
    """The 160 x 200 analytic image, 40 seeded points at least 40 px from the border, and the image moved by each shift."""
    H, W = 160, 200
    rng = np.random.default_rng(5)
    pts = np.c_[rng.uniform(40, W - 40, 40), rng.uniform(40, H - 40, 40)].astype(np.float32)
    return K.analytic_image(H, W), pts, {s: K.analytic_image(H, W, -s[0], -s[1]) for s in SHIFTS}


@pytest.mark.parametrize("shift", SHIFTS)
def test_reference_is_subpixel_on_the_analytic_image(analytic, shift):
    """Bounds that are structural, not measured: an integer-pixel answer is off by 0.38 px on average and by up to 0.71 px, so a
    median below 0.25 px and a maximum below 0.5 px say that the result is subpixel.  Measured: medians 0.013 -
    0.015 px, maxima 0.031 - 0.044 px."""
    a, pts, moved = analytic
    out = K.track(np.stack([a, moved[shift]]), [(0, 1)], [pts], max_level=3)
    assert (out["status"] == K.OK).all() and len(out["levels"][0]) == 3
    e = np.hypot(*(out["next"].astype(np.float64) - pts - np.array(shift)).T)
    print(f"shift {shift}: median {np.median(e):.4f} px, max {e.max():.4f} px")
    assert np.median(e) < 0.25 and e.max() < 0.5
    assert np.isfinite(out["err"]).all() and np.isnan(out["fb_err"]).all()


def test_the_pyramid_matters(analytic):
    a, pts, moved = analytic
    shift = SHIFTS[2]
    out = K.track(np.stack([a, moved[shift]]), [(0, 1)], [pts], max_level=0)
    e = np.hypot(*(out["next"].astype(np.float64) - pts - np.array(shift)).T)
    print(f"max_level 0 at shift {shift}: largest miss {e.max():.1f} px")
    assert e.max() > 1.0


def test_statuses_on_small_inputs():
    flat = np.full((2, 60, 70), 90, np.uint8)
    out = K.track(flat, [(0, 1)], [np.float32([[30, 30], [10.5, 40.25]])])
    assert out["status"].tolist() == [K.FLAT, K.FLAT] and np.isnan(out["err"]).all()
    assert np.array_equal(out["next"], np.float32([[30, 30], [10.5, 40.25]]))             # q never moved: next = (float)q = the start
    # a start outside, and a NaN start: OUT with next = prev
    # (the analytic image of the accuracy test, 120 wide.  Without a pyramid 8 px is at the edge of what a 21 px window follows:
    # there the iteration leaves the image on this seed and on five of the seven next ones, with the pyramid on all of them.)
    a = K.analytic_image(160, 120)
    b = K.analytic_image(160, 120, -8.0, 0.0)                        # the content moves 8 px towards the right border
    W = 120
    pts = np.float32([[W - 0.5, 50], [float("nan"), 50], [50, -0.25], [W - 1, 159]])
    out = K.track(np.stack([a, b]), [(0, 0)], [pts])
    assert out["status"].tolist() == [K.OUT, K.OUT, K.OUT, K.OK]                  # the corner pixel itself is inside
    assert np.array_equal(out["next"][[0, 2]], pts[[0, 2]]) and np.isnan(out["next"][1, 0]) and out["next"][1, 1] == 50
    assert np.abs(out["next"][3] - pts[3]).max() < 0.01 and out["err"][3] < 0.05 and np.isnan(out["err"][:3]).all()
    # a point whose content leaves the image, and one whose content stays
    for ml in (0, 2):
        info = []
        out = K.track(np.stack([a, b]), [(0, 1)], [np.float32([[115, 50], [60, 50]])], max_level=ml, info=info)
        assert out["status"].tolist() == [K.OUT, K.OK] and len(out["levels"][0]) == ml + 1
        assert info[0][-1]["level"] == 0 and info[0][-1]["exit"] == "out"
        assert np.isnan(out["err"][0]) and out["next"][0, 0] > W - 1               # next = (float)q, outside
        assert np.abs(out["next"][1].astype(np.float64) - [68.0, 50.0]).max() < 0.01
    # the forward-backward check on the same pair: the point that stays passes it with a tiny distance
    out = K.track(np.stack([a, b]), [(0, 1)], [np.float32([[60, 50], [115, 50]])], fb_max_px=0.5)
    assert out["status"].tolist() == [K.OK, K.OUT] and out["fb_err"][0] < 0.02 and np.isnan(out["fb_err"][1])
    out = K.track(np.stack([a, b]), [(0, 1)], [np.float32([[60, 50]])], fb_max_px=1e-9)
    assert out["status"].tolist() == [K.FB_FAIL] and np.isfinite(out["err"][0]) and out["fb_err"][0] > 1e-9


class _FakeSolver:
    """hip_backend.Solver.track_klt answered by the yardstick."""

    def __init__(self):
        self.calls = []

    def track_klt(self, images, pairs, points, guess=None, **opts):
        self.calls.append((np.asarray(images).shape, list(map(tuple, pairs)), guess is not None, opts))
        return K.track(images, pairs, points, guess=guess, **opts)


def test_features_host_side(lib):
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import features
    assert pkg.track is features.track and pkg.calc_optical_flow_pyr_lk is features.calc_optical_flow_pyr_lk
    assert pkg.refine_matches is features.refine_matches
    a = K.analytic_image(100, 120, seed=2)
    b = K.analytic_image(100, 120, -3.0, 2.0, seed=2)
    pts = np.float32([[60, 50], [40.5, 60.25], [119.5, 3]])
    fake = _FakeSolver()
    nxt, ok, err = features.track(a, b, pts, solver=fake, max_level=2)
    want = K.track(np.stack([a, b]), [(0, 1)], [pts], max_level=2)
    assert fake.calls[-1] == ((2, 100, 120), [(0, 1)], False, dict(max_level=2))
    assert np.array_equal(nxt, want["next"]) and ok.tolist() == [True, True, False] and ok.dtype == bool
    assert np.abs(nxt[:2].astype(np.float64) - pts[:2] - [3.0, -2.0]).max() < 0.05
    # cv2's shapes; colour goes through to_gray
    bgr = lambda g: np.stack([g, g, g], axis=2)
    p2, st, er = features.calc_optical_flow_pyr_lk(bgr(a), bgr(b), pts.reshape(-1, 1, 2), win_size=(21, 21), max_level=2, solver=fake)
    assert p2.shape == (3, 1, 2) and p2.dtype == np.float32 and st.shape == (3, 1) and st.dtype == np.uint8 and er.shape == (3, 1)
    assert np.array_equal(p2.reshape(-1, 2), nxt) and st.ravel().tolist() == [1, 1, 0]
    assert fake.calls[-1][3] == dict(half_window=10, max_level=2, max_iters=30, eps=0.01, min_eig=1e-4)
    for bad in ((21, 15), (20, 20), (21,)):
        with pytest.raises(ValueError):
            features.calc_optical_flow_pyr_lk(a, b, pts, win_size=bad, solver=fake)
    with pytest.raises(ValueError):
        features.track(a, b[:-1], pts, solver=fake)
    # refine_matches: kp1[q] tracked from the rounded kp2[t]; a match whose refinement runs away is dropped
    kp1 = np.float32([[60, 50], [40, 60], [30, 30]])
    kp2 = np.float32([[0, 0], [43, 58], [63, 48], [90, 90]])
    xy2, keep = features.refine_matches(a, kp1, b, kp2, [0, 1, 2], [2, 1, 3], solver=fake, max_level=0)
    assert fake.calls[-1][2] is True and keep.tolist() == [True, True, False]
    assert np.abs(xy2[:2].astype(np.float64) - kp1[:2] - [3.0, -2.0]).max() < 0.05 and np.array_equal(xy2[2], kp2[3])

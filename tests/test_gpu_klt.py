"""GPU: ba_track_klt (pyramid, window samples, Lucas-Kanade iterations and the forward-backward check on the device) against the
numpy yardstick of tests/klt_reference.py.  The definition sums integers and rounds every fp64 operation on its own, so every
comparison is exact equality: next, status and fb_err bit for bit, err with NaNs in the same places.

Shapes.  TW x TH = hip_backend.KLT_TILE_W x KLT_TILE_H is the tile of the pyramid kernel (a tile of the level it writes); an
image of 2 (TW + d) x 2 (TH + d), d = -1, 0, 1, puts the last column and row of level 1 one short of, on and one past a tile's
end.  The track kernel's split of a window over the lanes changes with half_window at 4 | 5, 7 | 8 and 10 | 11."""
import os

import numpy as np
import pytest

from tests import klt_reference as K
from tests import orb_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hb():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend


@pytest.fixture(scope="module")
def solver(hb):
    with hb.Solver(0) as s:
        yield s


def rolled(img, rows, cols):
    """(img, img rolled by (rows, cols)) stacked: the content moves by (dx, dy) = (cols, rows)."""
    return np.stack([img, np.roll(img, (rows, cols), axis=(0, 1))])


def points(seed, n, W, H, margin):
    rng = np.random.default_rng(seed)
    return np.c_[rng.uniform(margin, W - 1 - margin, n), rng.uniform(margin, H - 1 - margin, n)].astype(np.float32)


def check(solver, images, pairs, pts, guess=None, info=None, **opts):
    got = solver.track_klt(images, pairs, pts, guess=guess, **opts)
    want = K.track(images, pairs, pts, guess=guess, info=info, **opts)
    K.assert_equal(got, want)
    for g, w in zip(got["levels"], want["levels"]):
        assert g.tolist() == w.tolist()
    return got, want


# ---------------------------------------------------------------------------------------------------- 1: parity on texture
TEXTURE_CASES = [(10, 3), (3, 2), (1, 1), (15, 3)]


@pytest.fixture(scope="module")
def texture_refs():
    """The yardstick's result and per-level records for the four window / level cases, computed once."""
    imgs = rolled(R.texture(150, 200, 1), 3, -5)
    pts = points(7, 200, 200, 150, 12)
    out = {}
    for hw, ml in TEXTURE_CASES:
        info = []
        out[hw, ml] = (K.track(imgs, [(0, 1)], [pts], info=info, half_window=hw, max_level=ml), info)
    return imgs, pts, out


@pytest.mark.parametrize("hw,ml", TEXTURE_CASES)
def test_parity_texture(solver, texture_refs, hw, ml):
    imgs, pts, refs = texture_refs
    want = refs[hw, ml][0]
    got = solver.track_klt(imgs, [(0, 1)], [pts], half_window=hw, max_level=ml)
    K.assert_equal(got, want)
    assert got["levels"][0].tolist() == want["levels"][0].tolist() and got["levels"][1].tolist() == want["levels"][1].tolist()
    assert len(want["levels"][0]) == min(ml, 2) + 1                 # (at half_window 10 and 15 a fourth level would be below the window)
    assert (want["status"] == K.OK).sum() >= 100 if hw >= 10 else (want["status"] == K.OK).sum() >= 20


def test_texture_cases_take_every_exit(texture_refs):
    """The cases above do reach every branch of the definition: the three ways an iteration ends, a level left because the point
    ran out of the level image above level 0, and levels skipped as flat under the small windows."""
    refs = texture_refs[2]
    exits = {(r["exit"], r["level"] > 0) for _, info in refs.values() for rec in info for r in rec}
    assert {("eps", False), ("eps", True), ("osc", False), ("cap", False), ("out", True)} <= exits, exits
    assert {e for e, _ in exits} >= {"eps", "osc", "cap", "out", "skipped"}
    for key in ((3, 2), (1, 1)):
        assert any(r["exit"] == "skipped" for rec in refs[key][1] for r in rec), key
    statuses = set(np.concatenate([w["status"] for w, _ in refs.values()]).tolist())
    assert statuses >= {K.OK, K.OUT}


# ------------------------------------------------------------------------------------------------------- 2: real texture
def test_desk_crop_forward_backward(solver, golden_dir):
    img = np.load(os.path.join(golden_dir, "orb_desk_crop.npy"))
    assert img.shape == (224, 256)
    imgs = rolled(img, -2, 4)
    pts = points(11, 100, 256, 224, 12)
    got, want = check(solver, imgs, [(0, 1)], [pts], fb_max_px=0.5)
    # the check is what two plain calls with the roles swapped give
    fwd = solver.track_klt(imgs, [(0, 1)], [pts])
    ok = fwd["status"] == K.OK
    assert np.array_equal(fwd["next"].view(np.uint32), got["next"].view(np.uint32)) and ok.sum() >= 50
    back = solver.track_klt(imgs, [(1, 0)], [fwd["next"][ok]])
    dx = back["next"][:, 0].astype(np.float64) - pts[ok, 0].astype(np.float64)
    dy = back["next"][:, 1].astype(np.float64) - pts[ok, 1].astype(np.float64)
    u1 = dx * dx
    u2 = dy * dy
    dist = np.sqrt(u1 + u2)
    bad = (back["status"] != K.OK) | (dist > 0.5)
    status = fwd["status"].copy()
    status[np.nonzero(ok)[0][bad]] = K.FB_FAIL
    fb = np.full(len(pts), np.nan, np.float32)
    fb[np.nonzero(ok)[0][back["status"] == K.OK]] = dist[back["status"] == K.OK].astype(np.float32)
    assert np.array_equal(got["status"], status)
    assert np.array_equal(np.isnan(got["fb_err"]), np.isnan(fb)) and np.array_equal(got["fb_err"][~np.isnan(fb)], fb[~np.isnan(fb)])
    assert np.array_equal(got["err"][ok].view(np.uint32), fwd["err"][ok].view(np.uint32))
    # on the yardstick: what passes the check is right
    passed = want["status"] == K.OK
    miss = np.hypot(*(want["next"][passed].astype(np.float64) - pts[passed] - [4.0, -2.0]).T)
    print(f"{passed.sum()} of {len(pts)} pass the check; largest miss {miss.max():.3f} px")
    assert passed.sum() >= 50 and miss.max() < 1.0


# ------------------------------------------------------------------------------------------- 3: sizes around the geometry
def test_sizes_around_the_tiles(solver, hb):
    TW, TH = hb.KLT_TILE_W, hb.KLT_TILE_H
    for dw in (-1, 0, 1):
        for dh in (-1, 0, 1):
            W, H = 2 * (TW + dw), 2 * (TH + dh)
            imgs = rolled(R.texture(H, W, 20 + 3 * dw + dh, n_rect=12, noise=10), 1, -1)
            got, _ = check(solver, imgs, [(0, 1)], [points(3, 40, W, H, 2)], half_window=3)
            assert got["levels"][0].tolist() == [W, TW + dw] and got["levels"][1].tolist() == [H, TH + dh]
    # level 1 and level 2 both straddle tiles; the four instantiations of the track kernel at the borders of their ranges
    W, H = 4 * TW + 2, 4 * TH + 62                                 # level 2 is (TW + 1) x 24: room for a 23 x 23 window
    imgs = rolled(R.texture(H, W, 31), -1, 2)
    for hw in (4, 5, 7, 8, 11):
        got, _ = check(solver, imgs, [(0, 1)], [points(4, 60, W, H, 5)], half_window=hw, max_level=2)
        assert len(got["levels"][0]) == 3 and got["levels"][0][2] == TW + 1


@pytest.mark.parametrize("H,W,hw", [(61, 43, 10), (43, 61, 10), (21, 21, 10), (31, 31, 15), (3, 3, 1), (22, 47, 10)])
def test_odd_and_smallest_sizes(solver, H, W, hw):
    imgs = rolled(R.texture(H, W, 40 + H, n_rect=10, noise=12), 1, 1 if W > 3 else 0)
    pts = np.r_[points(5, 30, W, H, 0), np.float32([[0, 0], [W - 1, H - 1], [W // 2, H // 2]])]
    got, want = check(solver, imgs, [(0, 1)], [pts], half_window=hw)
    assert len(want["levels"][0]) == (2 if min(H, W) >= 41 else 1)


# ----------------------------------------------------------------------------------------------------- 4: special points
def test_special_points_and_guesses(solver):
    H, W = 90, 120
    imgs = rolled(R.texture(H, W, 5), 2, 3)                       # the content moves by (+3, +2)
    tiny = 2.0 ** -15
    base = np.float32([[40, 40], [0, 0], [W - 1, H - 1], [0, H - 1], [50 + tiny, 30], [50, 30 + tiny], [60 + tiny, 45 + tiny],
                       [33.5, 44.5], [W - 1 - tiny, 20], [70.25, 60.75]])
    assert float(base[4, 0]) != 50.0 and float(base[8, 0]) != W - 1           # the fractions survive float32
    check(solver, imgs, [(0, 1)], [base])
    check(solver, imgs, [(0, 1)], [base], max_level=0, half_window=4)
    pts = points(9, 40, W, H, 15)
    _, plain = check(solver, imgs, [(0, 1)], [pts])
    # an exact guess, a guess 30 px off, a guess outside the image and one that is no number
    exact = pts + np.float32([3, 2])
    _, want = check(solver, imgs, [(0, 1)], [pts], guess=[exact])
    good = plain["status"] == K.OK
    assert (want["status"][good] == K.OK).all() and np.abs(want["next"][good] - exact[good]).max() < 0.5
    off = pts + np.float32([30, 0])
    _, far = check(solver, imgs, [(0, 1)], [pts], guess=[off])
    assert (far["status"] != K.OK).any() or np.abs(far["next"] - exact).max() > 1.0      # (30 px is beyond two levels of this window)
    outside = pts.copy()
    outside[::2] = np.float32([W + 5.0, -3.0])
    outside[1] = np.float32([np.nan, 10.0])
    outside[3] = np.float32([np.inf, 10.0])
    info = []
    _, want = check(solver, imgs, [(0, 1)], [pts], guess=[outside], info=info)
    assert (want["status"][::2] == K.OUT).all() and want["status"][1] == K.OUT and want["status"][3] == K.OUT
    assert all(rec[-1]["level"] == 0 and rec[-1]["exit"] == "out" for rec in info[::2])       # OUT is decided at level 0
    assert np.isnan(want["err"][::2]).all()


# ----------------------------------------------------------------------------------------------------- 5: a skipped level
def test_skipped_levels(solver):
    rng = np.random.default_rng(17)
    img = np.clip(np.rint(128 + rng.normal(0, 40, (120, 140))), 0, 255).astype(np.uint8)
    imgs = rolled(img, 0, 1)
    pt = np.float32([[40, 40]])                                    # (a point whose level-1 value lies a third below that mean)
    info = []
    K.track(imgs, [(0, 1)], [pt], info=info, max_level=2)
    e = {r["level"]: r["e"] for r in info[0]}
    assert e[0] > e[1] > e[2] > 0                                  # the pyramid smooths noise away
    min_eig = float(np.sqrt(e[0] * e[2]))
    assert e[1] < min_eig < e[0]
    info = []
    _, want = check(solver, imgs, [(0, 1)], [pt], info=info, max_level=2, min_eig=min_eig)
    assert [(r["level"], r["exit"]) for r in info[0]][:2] == [(2, "skipped"), (1, "skipped")]
    assert info[0][2]["level"] == 0 and info[0][2]["exit"] in ("eps", "osc", "cap") and info[0][2]["iters"] >= 1
    assert want["status"].tolist() == [K.OK]
    # ... and with the bound above level 0 too, the point is FLAT where it started
    _, want = check(solver, imgs, [(0, 1)], [pt], max_level=2, min_eig=2.0 * e[0])
    assert want["status"].tolist() == [K.FLAT] and np.array_equal(want["next"], pt)


# ------------------------------------------------------------------------------------------------------------ 6: batching
def test_batching(solver):
    H, W = 80, 100
    t = R.texture(H, W, 8)
    imgs = np.stack([t, np.roll(t, (1, -2), axis=(0, 1)), R.texture(H, W, 9), R.texture(H, W, 10)])      # image 3 is in no pair
    pairs = [(0, 1), (1, 0), (2, 2), (0, 1), (2, 0)]
    pts = [points(1, 30, W, H, 5), points(2, 25, W, H, 5), points(3, 20, W, H, 0), points(4, 35, W, H, 5), np.zeros((0, 2), np.float32)]
    got, want = check(solver, imgs, pairs, pts, fb_max_px=1.0)
    assert got["pt_off"].tolist() == [0, 30, 55, 75, 110, 110]
    for k, (pr, p) in enumerate(zip(pairs, pts)):
        one = solver.track_klt(imgs, [pr], [p], fb_max_px=1.0)
        lo, hi = int(got["pt_off"][k]), int(got["pt_off"][k + 1])
        for key in ("next", "err", "fb_err"):
            assert np.array_equal(one[key].view(np.uint32), got[key][lo:hi].view(np.uint32)), (k, key)
        assert np.array_equal(one["status"], got["status"][lo:hi])
    same = want["status"][55:75] == K.OK                            # an image against itself: the points stay
    assert same.sum() >= 5 and np.abs(want["next"][55:75][same] - pts[2][same]).max() < 0.01
    # only pairs without points, and no pair at all
    for pr, p in (([(0, 1), (3, 3)], [pts[4], pts[4]]), ([], [])):
        out = solver.track_klt(imgs, np.array(pr, np.int32).reshape(-1, 2), p)
        assert len(out["next"]) == 0 and len(out["status"]) == 0 and out["pt_off"].tolist() == [0] * (len(pr) + 1)


# --------------------------------------------------------------------------------------------------------------- 7: arena
def test_arena(solver, hb):
    H, W = 90, 120
    imgs = rolled(R.texture(H, W, 12), 1, 2)
    pts = points(6, 80, W, H, 3)
    kw = dict(fb_max_px=0.5)

    def bits(out):
        return [out[k].view(np.uint32 if out[k].dtype == np.float32 else np.uint8).copy() for k in ("next", "status", "err", "fb_err")]

    first = bits(solver.track_klt(imgs, [(0, 1)], [pts], **kw))
    for byte in (0xff, 0x00):
        solver.debug_scratch_fill(byte)
        again = bits(solver.track_klt(imgs, [(0, 1)], [pts], **kw))
        assert all(np.array_equal(a, b) for a, b in zip(first, again)), byte
    allocs = solver.stats()["scratch_allocs"]
    for _ in range(3):
        again = bits(solver.track_klt(imgs, [(0, 1)], [pts], **kw))
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
    assert solver.stats()["scratch_allocs"] == allocs
    # an ORB extraction and a match in between leave nothing behind that the tracker reads
    orb = solver.extract_orb(R.texture(150, 200, 1), n_levels=2, n_features=300)
    assert int(orb["n_kp"][0]) > 20
    solver.match_descriptors([orb["desc"], orb["desc"][::-1].copy()])
    again = bits(solver.track_klt(imgs, [(0, 1)], [pts], **kw))
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    with hb.Solver(0) as fresh:
        again = bits(fresh.track_klt(imgs, [(0, 1)], [pts], **kw))
    assert all(np.array_equal(a, b) for a, b in zip(first, again))


# ---------------------------------------------------------------------------------------------------------- 8: end to end
def test_refine_matches_end_to_end(solver):
    from bundle_adjustment_amd import features
    H, W, shift = 160, 200, np.array([3.3, 2.6])
    a, b = K.analytic_image(H, W), K.analytic_image(H, W, -shift[0], -shift[1])
    kp = features.extract(a, solver=solver, n_levels=1, n_features=200, fast_threshold=8)
    kp1 = kp["xy"]
    assert len(kp1) >= 20
    truth = kp1.astype(np.float64) + shift
    kp2 = np.rint(truth).astype(np.float32)                     # what an integer-pixel detector would report in image 2
    idx = np.arange(len(kp1))
    xy2, keep = features.refine_matches(a, kp1, b, kp2, idx, idx, solver=solver)
    assert keep.sum() >= 0.9 * len(kp1)
    refined, rounded = np.hypot(*(xy2[keep] - truth[keep]).T), np.hypot(*(kp2[keep] - truth[keep]).T)
    print(f"{keep.sum()} of {len(kp1)} kept; refined: median {np.median(refined):.4f}, max {refined.max():.4f} px; rounded: median {np.median(rounded):.4f} px")
    assert np.median(refined) < 0.25 and refined.max() < 0.5 and (refined < rounded).all()
    # the drop-in: cv2's shapes, status 1 exactly where the status is OK
    pts = np.r_[kp1[:30], np.float32([[W - 0.5, 10], [-1, 5]])]
    want = K.track(np.stack([a, b]), [(0, 1)], [pts])
    p2, st, err = features.calc_optical_flow_pyr_lk(a, b, pts.reshape(-1, 1, 2), solver=solver)
    assert p2.shape == (32, 1, 2) and p2.dtype == np.float32 and st.shape == (32, 1) and st.dtype == np.uint8 and err.shape == (32, 1)
    assert np.array_equal(st.ravel() == 1, want["status"] == K.OK) and st[-2:].ravel().tolist() == [0, 0] and st.sum() >= 25
    assert np.array_equal(p2.reshape(-1, 2).view(np.uint32), want["next"].view(np.uint32))
    nxt, ok, _ = features.track(a, b, pts, solver=solver)
    assert np.array_equal(ok, want["status"] == K.OK) and np.array_equal(nxt.view(np.uint32), want["next"].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_and_resident_problem(solver, hb):
    from bundle_adjustment_amd.synthetic import make_problem
    H, W = 60, 70
    imgs = rolled(R.texture(H, W, 2, n_rect=10), 1, 1)
    pts = points(1, 10, W, H, 3)
    prob = make_problem(6, 200, 4, seed=1)
    solver.set_problem(prob)
    r0 = solver.residuals("huber")
    ok = solver.track_klt(imgs, [(0, 1)], [pts])
    import ctypes as C
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    o = hb.klt_options()
    bp = C.POINTER(C.c_uint8)

    def raw(n_images=2, n_pairs=1, pairs=((0, 1),), pt_off=(0, 10), images=imgs, prev=pts, opts=o, height=H, width=W):
        pr = np.array(pairs, np.int32).reshape(-1, 2)
        off = np.array(pt_off, np.int64)
        nxt = np.zeros((16, 2), np.float32)                       # (room for the ten points of the calls that are not refused)
        rc = solver._lib.ba_track_klt(solver._h, n_images, height, width, None if images is None else images.ctypes.data_as(bp), n_pairs,
                                      pr.ctypes.data_as(ip), off.ctypes.data_as(C.POINTER(C.c_int64)),
                                      None if prev is None else prev.ctypes.data_as(fp), None, C.byref(opts), nxt.ctypes.data_as(fp), None, None, None)
        return rc, solver._lib.ba_last_error().decode()

    assert raw()[0] == 0
    for kw, word in ((dict(pairs=((0, 2),)), "pairs"), (dict(pairs=((-1, 1),)), "pairs"), (dict(pt_off=(1, 10)), "pt_off"),
                     (dict(n_pairs=2, pairs=((0, 1), (1, 0)), pt_off=(0, 10, 5)), "pt_off"), (dict(n_pairs=-1), "n_pairs"),
                     (dict(n_pairs=65536), "n_pairs"), (dict(n_images=-1), "n_images"), (dict(n_images=1025), "n_images"),
                     (dict(images=None), "images"), (dict(prev=None), "prev"), (dict(pt_off=(0, (1 << 24) + 1)), "points"),
                     (dict(height=1 << 14, width=(1 << 12) + 1), "cap"), (dict(n_images=1024, height=1 << 10, width=(1 << 8) + 1), "cap"),
                     (dict(opts=hb.klt_options(half_window=16)), "half_window"), (dict(opts=hb.klt_options(max_iters=0)), "max_iters"),
                     (dict(height=20), "window")):
        rc, msg = raw(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    with pytest.raises(hb.BAHipError, match="eps"):
        solver.track_klt(imgs, [(0, 1)], [pts], eps=-1.0)
    with pytest.raises(ValueError):
        solver.track_klt(imgs, [(0, 1)], [pts, pts])
    with pytest.raises(ValueError):
        solver.track_klt(imgs.astype(np.float32), [(0, 1)], [pts])
    # a refused call leaves the handle usable, two calls give equal bits, and the resident problem is as it was
    again = solver.track_klt(imgs, [(0, 1)], [pts])
    for k in ("next", "err"):
        assert np.array_equal(ok[k].view(np.uint32), again[k].view(np.uint32))
    r1 = solver.residuals("huber")
    assert np.array_equal(r0[0], r1[0]) and r0[1:] == r1[1:]

"""CPU: the yardstick of the ORB tests (tests/orb_reference.py) against slow literal loops, its rotation property, and the
surface of ba_orb_extract that needs no device: the level function, the default pattern, the options struct, features.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import orb_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from bundle_adjustment_amd import hip_backend
    return hip_backend.load_library()


texture = R.texture


@pytest.fixture(scope="module")
def img40():
    return texture(40, 40, 7, n_rect=12, noise=10)


def test_fast_score_and_suppression_against_loops(img40):
    I = img40.astype(int)
    h, w = I.shape
    S = np.zeros((h, w), int)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            ring = [I[y + dy, x + dx] for dx, dy in R.RING]
            best = -10 ** 9
            for a in range(16):
                arc = [ring[(a + j) % 16] for j in range(9)]
                best = max(best, min(r - I[y, x] for r in arc), min(I[y, x] - r for r in arc))
            S[y, x] = best
    assert np.array_equal(R.fast_scores(img40), S)
    thr = 12
    want = np.zeros((h, w), int)
    for y in range(h):
        for x in range(w):
            if S[y, x] <= thr:
                continue
            ok = True
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dx or dy) and 0 <= y + dy < h and 0 <= x + dx < w:
                        n = S[y + dy, x + dx]
                        ok = ok and S[y, x] > (n if n > thr else 0)
            want[y, x] = S[y, x] if ok else 0
    got = R.corners(img40, thr)
    assert np.array_equal(got, want) and (want > 0).sum() >= 3
    # the segment test: a pixel is a corner at threshold t exactly when its score exceeds t
    for t in (5, 12, 30):
        for y in range(3, h - 3):
            for x in range(3, w - 3):
                ring = [I[y + dy, x + dx] for dx, dy in R.RING]
                seg = any(all(ring[(a + j) % 16] > I[y, x] + t for j in range(9)) or all(ring[(a + j) % 16] < I[y, x] - t for j in range(9))
                          for a in range(16))
                assert seg == (S[y, x] > t)


def test_harris_moments_blur_against_loops(img40):
    I = img40.astype(int)
    pts = [(17, 18), (20, 22), (16, 23), (24, 16)]
    xs, ys = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    hs = R.harris(img40, xs, ys)
    m10, m01 = R.moments(img40, xs, ys)
    for k, (x, y) in enumerate(pts):
        a = b = c = 0
        for dy in range(-3, 4):
            for dx in range(-3, 4):
                X, Y = x + dx, y + dy
                ix = 2 * (I[Y, X + 1] - I[Y, X - 1]) + (I[Y - 1, X + 1] - I[Y - 1, X - 1]) + (I[Y + 1, X + 1] - I[Y + 1, X - 1])
                iy = 2 * (I[Y + 1, X] - I[Y - 1, X]) + (I[Y + 1, X - 1] - I[Y - 1, X - 1]) + (I[Y + 1, X + 1] - I[Y - 1, X + 1])
                a, b, c = a + ix * ix, b + iy * iy, c + ix * iy
        assert int(hs[k]) == 25 * (a * b - c * c) - (a + b) ** 2
        s10 = s01 = 0
        for v in range(-15, 16):
            for u in range(-R.UMAX[abs(v)], R.UMAX[abs(v)] + 1):
                s10 += u * I[y + v, x + u]
                s01 += v * I[y + v, x + u]
        assert (int(m10[k]), int(m01[k])) == (s10, s01)
    B = R.blur(img40)
    for y in range(3, 37):
        for x in range(3, 37):
            t = [sum(R.GAUSS[k] * I[y + j - 3, x + k - 3] for k in range(7)) for j in range(7)]
            assert max(t) < 65536
            assert int(B[y, x]) == (sum(R.GAUSS[j] * t[j] for j in range(7)) + 32768) >> 16
    assert sum(R.GAUSS) == 256


def test_resize_against_float_bilinear():
    img = texture(60, 90, 3)
    for (wd, hd) in ((75, 50), (45, 30), (89, 59)):
        got = R.resize(img, wd, hd).astype(float)
        sx = (np.arange(wd) + 0.5) * (90 / wd) - 0.5
        sy = (np.arange(hd) + 0.5) * (60 / hd) - 0.5
        x0, y0 = np.floor(sx).astype(int), np.floor(sy).astype(int)
        fx, fy = sx - x0, sy - y0
        x0c, x1c = np.clip(x0, 0, 89), np.clip(x0 + 1, 0, 89)
        y0c, y1c = np.clip(y0, 0, 59), np.clip(y0 + 1, 0, 59)
        F = img.astype(float)
        want = ((1 - fy)[:, None] * ((1 - fx)[None] * F[y0c][:, x0c] + fx[None] * F[y0c][:, x1c]) +
                fy[:, None] * ((1 - fx)[None] * F[y1c][:, x0c] + fx[None] * F[y1c][:, x1c]))
        assert np.abs(got - want).max() <= 1.0


LEVEL_CASES = [(720, 1280, 1.2, 8, 3000), (135, 195, 1.2, 4, 500), (150, 200, 1.2, 4, 500), (480, 640, 1.5, 5, 1000), (90, 135, 1.2, 3, 7),
               (100, 100, 2.0, 16, 100), (64, 64, 1.2, 1, 40), (480, 640, 1.2, 8, 7), (300, 415, 1.1, 12, 65536)]


@pytest.mark.parametrize("H,W,sf,L,N", LEVEL_CASES)
def test_levels_equal_the_reference(lib, H, W, sf, L, N):
    from bundle_adjustment_amd import hip_backend as hb
    got = hb.orb_levels(H, W, scale_factor=sf, n_levels=L, n_features=N)
    want = R.levels(H, W, scale_factor=sf, n_levels=L, n_features=N)
    for g, w_ in zip(got, want):
        assert g.dtype == w_.dtype and np.array_equal(g, w_)
    assert int(got[3].sum()) == N and (got[3] >= 0).all()
    assert got[0][0] == W and got[1][0] == H and got[2][0] == 1.0


def test_quotas_sum_to_n_features_for_small_n(lib):
    """Rounding every level's share on its own would overshoot for a small n_features (7 features over 8 levels at 1.2 would be
    2 1 1 1 1 1 1 0 = 8): the quotas are capped by what is left, so they sum to n_features and n_kp never exceeds it."""
    from bundle_adjustment_amd import hip_backend as hb
    assert R.levels(480, 640, n_levels=8, n_features=7)[3].tolist() == [2, 1, 1, 1, 1, 1, 0, 0]
    capped = 0
    for sf in (1.1, 1.2, 1.5):
        for L in range(2, 17):
            f = 1.0 / sf
            for N in range(1, 200):
                q = hb.orb_levels(480, 640, scale_factor=sf, n_levels=L, n_features=N)[3]
                assert int(q.sum()) == N and (q >= 0).all(), (sf, L, N, q)
                assert np.array_equal(q, R.levels(480, 640, scale_factor=sf, n_levels=L, n_features=N)[3])
                d, raw = N * (1.0 - f) / (1.0 - f ** L), 0
                for _ in range(L - 1):
                    raw, d = raw + int(np.rint(d)), d * f
                capped += raw > N
    assert capped > 100            # (the sweep does hold cases where the cap binds)


def test_levels_round_half_to_even(lib):
    from bundle_adjustment_amd import hip_backend as hb
    # 195 / 1.2 = 162.5 and 135 / 1.2 = 112.5 exactly in fp64 terms of the quotient's rounding: half goes to the even side
    assert 195 / 1.2 == 162.5 and 135 / 1.2 == 112.5
    w, h, _, _ = hb.orb_levels(135, 195, n_levels=2)
    assert (int(w[1]), int(h[1])) == (162, 112)
    with pytest.raises(hb.BAHipError, match="n_levels"):
        hb.orb_levels(100, 100, n_levels=17)
    with pytest.raises(hb.BAHipError, match="scale_factor"):
        hb.orb_levels(100, 100, scale_factor=1.0)
    with pytest.raises(hb.BAHipError, match="width"):
        hb.orb_levels(100, 0)


def test_default_pattern(lib):
    from bundle_adjustment_amd import hip_backend as hb
    raw = (C.c_int8 * 1024)()
    assert lib.ba_orb_default_pattern(raw) == 0
    pat = hb.orb_default_pattern()
    assert pat.shape == (256, 4) and pat.dtype == np.int8
    assert np.array_equal(np.frombuffer(raw, dtype=np.int8).reshape(256, 4), pat)
    assert np.abs(pat).max() <= 13
    assert not ((pat[:, 0] == pat[:, 2]) & (pat[:, 1] == pat[:, 3])).any()
    assert len({tuple(r) for r in pat.tolist()}) == 256
    assert lib.ba_orb_default_pattern(None) == -1 and b"null" in lib.ba_last_error()
    # the table lives in one place: the C++ header
    src = open(os.path.join(ROOT, "bundle_adjustment_amd", "csrc", "ba_orb.hpp")).read()
    body = re.search(r"kOrbDefaultPattern\[256\]\[4\] = \{(.*?)\};", src, flags=re.S).group(1)
    assert np.array_equal(np.array([int(v) for v in re.findall(r"-?\d+", body)]).reshape(256, 4), pat)


def test_abi(lib):
    from bundle_adjustment_amd import hip_backend as hb
    for name in ("ba_default_orb_options", "ba_orb_default_pattern", "ba_orb_levels", "ba_orb_extract"):
        assert hasattr(lib, name) and name in hb.SYMBOLS
    o = hb.BAOrbOptions()
    assert lib.ba_default_orb_options(C.byref(o)) == 0
    assert (o.scale_factor, o.n_features, o.n_levels, o.edge_threshold, o.fast_threshold) == (1.2, 3000, 8, 31, 20)
    assert C.sizeof(hb.BAOrbOptions) == 24
    off = {k: getattr(hb.BAOrbOptions, k).offset for k, _ in hb.BAOrbOptions._fields_}
    assert off == dict(scale_factor=0, n_features=8, n_levels=12, edge_threshold=16, fast_threshold=20)
    hdr = open(os.path.join(ROOT, "include", "ba_hip.h")).read()
    body = re.search(r"typedef struct ba_orb_options \{(.*?)\} ba_orb_options;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(int32_t|double)\s+([a-z_0-9]+)\s*;", body)
    ctype = {"double": C.c_double, "int32_t": C.c_int32}
    assert [(n, ctype[t]) for t, n in fields] == list(hb.BAOrbOptions._fields_)
    assert lib.ba_default_orb_options(None) == -1 and b"null" in lib.ba_last_error()
    src = open(os.path.join(ROOT, "bundle_adjustment_amd", "csrc", "ba_orb.hpp")).read()
    consts = {k: int(v) for k, v in re.findall(r"constexpr int (ORB_[A-Z_]+) = (\d+);", src)}
    assert (consts["ORB_TILE_W"], consts["ORB_TILE_H"], consts["ORB_MAX_LEVELS"]) == (hb.ORB_TILE_W, hb.ORB_TILE_H, hb.ORB_MAX_LEVELS)
    with pytest.raises(TypeError):
        hb.orb_options(wta_k=3)


class _FakeSolver:
    """hip_backend.Solver.extract_orb answered by the yardstick."""

    def __init__(self):
        self.calls = []

    def extract_orb(self, images, pattern=None, **opts):
        from bundle_adjustment_amd import hip_backend as hb
        self.calls.append((np.asarray(images).shape, pattern, opts))
        return R.extract(images, hb.orb_default_pattern() if pattern is None else pattern, **opts)


def test_extractor_host_side(lib):
    import bundle_adjustment_amd as pkg
    from bundle_adjustment_amd import features
    assert pkg.ORBExtractor is features.ORBExtractor
    assert features.KeyPoint.__slots__ == ("pt", "size", "angle", "response", "octave", "class_id")
    fake = _FakeSolver()
    ex = features.ORBExtractor(n_features=60, solver=fake, n_levels=2)
    assert ex.extract(np.full((90, 90), 7, np.uint8)) == ([], None)
    assert fake.calls[-1] == ((90, 90), None, dict(n_features=60, n_levels=2))
    img = texture(110, 130, 5)
    kps, des = ex.extract(img)
    ref = R.extract(img, fake.calls[-1][1] if fake.calls[-1][1] is not None else __import__("bundle_adjustment_amd").hip_backend.orb_default_pattern(),
                    n_features=60, n_levels=2)
    assert len(kps) == len(des) == int(ref["n_kp"][0]) > 10 and des.dtype == np.uint8 and des.shape[1] == 32
    assert np.array_equal(des, ref["desc"])
    for k, kp in enumerate(kps):
        assert kp.pt == (float(ref["xy"][k, 0]), float(ref["xy"][k, 1])) and type(kp.pt[0]) is float
        assert (kp.size, kp.angle, kp.response, kp.octave, kp.class_id) == \
            (float(ref["size"][k]), float(ref["angle"][k]), float(ref["response"][k]), int(ref["octave"][k]), -1)
        assert type(kp.octave) is int and 0.0 <= kp.angle < 360.0
    assert {kp.octave for kp in kps} == {0, 1}
    # a colour image goes through to_gray; the batch form returns the arrays
    bgr = np.stack([img, img, img], axis=2)
    kps2, des2 = ex.extract(bgr)
    assert np.array_equal(des2, des) and [k.pt for k in kps2] == [k.pt for k in kps]
    out = features.extract(np.stack([img, img[::-1].copy()]), solver=fake, n_features=60, n_levels=2)
    assert out["kp_off"].tolist()[0] == 0 and len(out["kp_off"]) == 3 and np.array_equal(out["desc"][:len(des)], des)
    # estimate_pose and the guided matchers read .pt
    assert features._positions(kps).shape == (len(kps), 2)


def test_to_gray():
    from bundle_adjustment_amd.features import to_gray
    px = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0]], [[0, 0, 255], [10, 20, 30], [1, 1, 1], [200, 100, 50]]], np.uint8)
    want = [[0, 255, (1868 * 255 + 8192) >> 14, (9617 * 255 + 8192) >> 14],
            [(4899 * 255 + 8192) >> 14, (1868 * 10 + 9617 * 20 + 4899 * 30 + 8192) >> 14, 1, (1868 * 200 + 9617 * 100 + 4899 * 50 + 8192) >> 14]]
    assert to_gray(px).tolist() == want and to_gray(px).dtype == np.uint8
    assert want[0][2:] == [29, 150] and want[1][0] == 76
    g = np.zeros((3, 4), np.uint8)
    assert to_gray(g) is g
    with pytest.raises(ValueError):
        to_gray(px.astype(np.float32))


def test_rotation_property_of_the_reference(lib):
    """One level, quotas not binding: np.rot90 maps the keypoint set exactly, shifts the angles by 90 degrees and leaves the
    multiset of descriptors as it is (the ring, the patch, the Harris block and the blur weights are symmetric under the rotation)."""
    from bundle_adjustment_amd import hip_backend as hb
    R.check_rotation(lambda im, **kw: R.extract(im, hb.orb_default_pattern(), **kw))

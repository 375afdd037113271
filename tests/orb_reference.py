"""Yardstick of the ORB extraction tests: a vectorised numpy restatement of the definition in include/ba_hip.h (ba_orb_extract).
Every stage is integer arithmetic or float64 with each operation rounded on its own, so the device must agree exactly (the
angle, which goes through atan2, within 1e-4 degrees).  tests/test_orb_host.py checks the stages against literal loops."""
import numpy as np

RING = ((0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1),
        (-2, -2), (-1, -3))
UMAX = (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)
GAUSS = (18, 34, 49, 54, 49, 34, 18)
DEFAULTS = dict(scale_factor=1.2, n_features=3000, n_levels=8, edge_threshold=31, fast_threshold=20)
HARRIS_NORM = 2598919616160000.0      # 7140^4


def levels(height, width, scale_factor=1.2, n_features=3000, n_levels=8, **_):
    """-> (level_w, level_h int32 (L,), level_scale float64 (L,), level_quota int32 (L,))."""
    sf = float(scale_factor)
    L = int(n_levels)
    w, h, sc, q = np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros(L, np.float64), np.zeros(L, np.int32)
    s = 1.0
    for l in range(L):
        if l > 0:
            s = s * sf
        sc[l] = s
        w[l] = int(np.rint(float(width) / s))
        h[l] = int(np.rint(float(height) / s))
    f = 1.0 / sf
    p = 1.0
    for _ in range(L):
        p = p * f
    if L == 1:
        q[0] = n_features
    else:
        d = float(n_features) * (1.0 - f) / (1.0 - p)
        tot = 0
        for l in range(L - 1):
            q[l] = min(int(np.rint(d)), int(n_features) - tot)      # the quotas never sum to more than n_features
            tot += int(q[l])
            d = d * f
        q[L - 1] = int(n_features) - tot
    return w, h, sc, q


def _axis(n_src, n_dst):
    """Source indices and the 11-bit weight of the second one, for every destination index along one axis."""
    ratio = float(n_src) / float(n_dst)
    s = (np.arange(n_dst, dtype=np.float64) + 0.5) * ratio - 0.5
    i0 = np.floor(s)
    f = s - i0
    i0 = i0.astype(np.int64)
    clamped = (i0 < 0) | (i0 > n_src - 1)
    f = np.where(clamped, 0.0, f)
    i1 = np.clip(i0 + 1, 0, n_src - 1)
    i0 = np.clip(i0, 0, n_src - 1)
    a1 = np.rint(f * 2048.0).astype(np.int64)
    return i0, i1, a1


def resize(img, w_dst, h_dst):
    h, w = img.shape
    x0, x1, ax = _axis(w, w_dst)
    y0, y1, ay = _axis(h, h_dst)
    I = img.astype(np.int64)
    bx0, bx1, by0, by1 = (2048 - ax)[None, :], ax[None, :], (2048 - ay)[:, None], ay[:, None]
    acc = (by0 * bx0 * I[y0][:, x0] + by0 * bx1 * I[y0][:, x1] + by1 * bx0 * I[y1][:, x0] + by1 * bx1 * I[y1][:, x1])
    return ((acc + (1 << 21)) >> 22).astype(np.uint8)


def pyramid(img, lw, lh):
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for l in range(1, len(lw)):
        empty = lw[l] == 0 or lh[l] == 0                 # (a level of no pixels: nothing to resize, and nothing above it)
        out.append(np.zeros((int(lh[l]), int(lw[l])), np.uint8) if empty else resize(out[-1], int(lw[l]), int(lh[l])))
    return out


def fast_scores(img):
    """The FAST-9 score of every pixel whose ring lies in the image (int32; 0 elsewhere)."""
    I = img.astype(np.int32)
    h, w = I.shape
    S = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return S
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    d = np.concatenate([d, d[:8]])
    best = np.full(c.shape, -255, np.int32)
    for a in range(16):
        arc = d[a:a + 9]
        best = np.maximum(best, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    S[3:h - 3, 3:w - 3] = best
    return S


def corners(img, fast_threshold):
    """Score where the pixel is a corner that survives the suppression, 0 elsewhere (no domain applied)."""
    S = fast_scores(img)
    S = np.where(S > fast_threshold, S, 0)
    P = np.pad(S, 1)
    h, w = S.shape
    keep = S > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                keep &= S > P[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    return np.where(keep, S, 0)


def candidates(img, fast_threshold, edge):
    """-> (raster index int64, score int32) of the candidates, in raster order."""
    S = corners(img, fast_threshold)
    h, w = S.shape
    D = np.zeros_like(S)
    if w > 2 * edge and h > 2 * edge:
        D[edge:h - edge, edge:w - edge] = S[edge:h - edge, edge:w - edge]
    r = np.nonzero(D.ravel())[0]
    return r.astype(np.int64), D.ravel()[r]


def harris(img, xs, ys):
    I = np.pad(img.astype(np.int64), 1)
    h, w = img.shape
    def at(dx, dy):
        return I[1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    Ix = 2 * (at(1, 0) - at(-1, 0)) + (at(1, -1) - at(-1, -1)) + (at(1, 1) - at(-1, 1))
    Iy = 2 * (at(0, 1) - at(0, -1)) + (at(-1, 1) - at(-1, -1)) + (at(1, 1) - at(1, -1))
    o = np.arange(-3, 4)
    yy = ys[:, None, None] + o[None, :, None]
    xx = xs[:, None, None] + o[None, None, :]
    gx, gy = Ix[yy, xx], Iy[yy, xx]
    a, b, c = (gx * gx).sum(axis=(1, 2)), (gy * gy).sum(axis=(1, 2)), (gx * gy).sum(axis=(1, 2))
    return 25 * (a * b - c * c) - (a + b) * (a + b)


def moments(img, xs, ys):
    o = np.arange(-15, 16)
    mask = np.abs(o)[None, :] <= np.array(UMAX)[np.abs(o)][:, None]       # [v][u]
    P = img.astype(np.int64)[ys[:, None, None] + o[None, :, None], xs[:, None, None] + o[None, None, :]] * mask[None]
    return (P * o[None, None, :]).sum(axis=(1, 2)), (P * o[None, :, None]).sum(axis=(1, 2))


def blur(img):
    """The 7x7 integer Gaussian; pixels within 3 of a border are left 0 (never read)."""
    h, w = img.shape
    out = np.zeros((h, w), np.uint8)
    if h < 7 or w < 7:
        return out
    I = img.astype(np.int64)
    t = sum(GAUSS[k] * I[:, k:w - 6 + k] for k in range(7))
    v = sum(GAUSS[k] * t[k:h - 6 + k] for k in range(7))
    out[3:h - 3, 3:w - 3] = (v + 32768) >> 16
    return out


def steer(m10, m01):
    """-> (c, s) float64 and the angle in degrees, float32 in [0, 360)."""
    m10, m01 = m10.astype(np.int64), m01.astype(np.int64)
    r = np.sqrt((m10 * m10 + m01 * m01).astype(np.float64))
    zero = r == 0.0
    rr = np.where(zero, 1.0, r)
    c = np.where(zero, 1.0, m10.astype(np.float64) / rr)
    s = np.where(zero, 0.0, m01.astype(np.float64) / rr)
    a = np.arctan2(m01.astype(np.float64), m10.astype(np.float64)) * (180.0 / np.pi)
    a = np.where(a < 0, a + 360.0, a).astype(np.float32)
    a = np.where(a >= np.float32(360.0), np.float32(0.0), a).astype(np.float32)
    return c, s, a


def describe(B, xs, ys, c, s, pattern):
    p = np.asarray(pattern, dtype=np.float64).reshape(256, 4)
    c, s = c[:, None], s[:, None]
    val = []
    for k in (0, 2):
        px, py = p[None, :, k], p[None, :, k + 1]
        u = np.rint(px * c - py * s).astype(np.int64)
        v = np.rint(px * s + py * c).astype(np.int64)
        val.append(B[ys[:, None] + v, xs[:, None] + u].astype(np.int64))
    bits = (val[0] < val[1]).astype(np.uint8).reshape(len(xs), 32, 8)
    return (bits << np.arange(8, dtype=np.uint8)[None, None, :]).sum(axis=2).astype(np.uint8)


def extract_level(img, n_l, pattern, edge_threshold, fast_threshold, info=None):
    """One level image -> (x, y, Hs, c, s, angle, desc) of its keypoints in output order."""
    h, w = img.shape
    r, sc = candidates(img, fast_threshold, edge_threshold)
    order = np.lexsort((r, -sc.astype(np.int64)))
    if info is not None:
        info["stage1_scores"] = sc[order]
    order = order[:2 * n_l]
    r = r[order]
    xs, ys = r % w, r // w
    Hs = harris(img, xs, ys) if len(r) else np.zeros(0, np.int64)
    o2 = np.lexsort((r, -Hs))
    if info is not None:
        info["stage2_hs"] = Hs[o2]
    o2 = o2[:n_l]
    xs, ys, Hs = xs[o2], ys[o2], Hs[o2]
    if len(xs) == 0:
        z = np.zeros(0)
        return xs, ys, Hs, z, z, z.astype(np.float32), np.zeros((0, 32), np.uint8)
    m10, m01 = moments(img, xs, ys)
    c, s, ang = steer(m10, m01)
    return xs, ys, Hs, c, s, ang, describe(blur(img), xs, ys, c, s, pattern)


def extract(images, pattern, info=None, **opts):
    """images (n, H, W) or (H, W) uint8 -> the dict of hip_backend.Solver.extract_orb (arrays compacted per image, kp_off).
    info: a list that receives, per (image, level), a dict of the stage-1 scores and stage-2 Hs values in sorted order."""
    o = dict(DEFAULTS, **opts)
    imgs = np.asarray(images)
    if imgs.ndim == 2:
        imgs = imgs[None]
    n, H, W = imgs.shape
    lw, lh, ls, lq = levels(H, W, **o)
    cols = dict(xy=[], size=[], angle=[], response=[], octave=[], level_xy=[], cs=[], desc=[])
    kp_off = [0]
    for b in range(n):
        pyr = pyramid(imgs[b], lw, lh)
        cnt = 0
        for l, img in enumerate(pyr):
            rec = {} if info is not None else None
            xs, ys, Hs, c, s, ang, desc = extract_level(img, int(lq[l]), pattern, o["edge_threshold"], o["fast_threshold"], rec)
            if info is not None:
                info.append(rec)
            m = len(xs)
            cnt += m
            cols["xy"].append(np.stack([(xs.astype(np.float64) * ls[l]), (ys.astype(np.float64) * ls[l])], axis=1).astype(np.float32).reshape(m, 2))
            cols["size"].append(np.full(m, np.float32(31.0 * ls[l]), np.float32))
            cols["angle"].append(ang.astype(np.float32))
            cols["response"].append(((Hs.astype(np.float64) / 25.0) / HARRIS_NORM).astype(np.float32))
            cols["octave"].append(np.full(m, l, np.int32))
            cols["level_xy"].append(np.stack([xs, ys], axis=1).astype(np.int32).reshape(m, 2))
            cols["cs"].append(np.stack([c, s], axis=1).astype(np.float64).reshape(m, 2))
            cols["desc"].append(desc.reshape(m, 32))
        kp_off.append(kp_off[-1] + cnt)
    out = {k: np.concatenate(v, axis=0) for k, v in cols.items()}
    out["kp_off"] = np.array(kp_off, dtype=np.int64)
    out["n_kp"] = np.diff(out["kp_off"]).astype(np.int32)
    return out


# ------------------------------------------------------------------------------ shared by the CPU and the GPU tests
def texture(h, w, seed, n_rect=40, noise=6):
    """Seeded random rectangles, blobs and noise."""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 100.0)
    for _ in range(n_rect):
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        img[y0:y0 + int(rng.integers(4, 30)), x0:x0 + int(rng.integers(4, 30))] = float(rng.integers(0, 256))
    yy, xx = np.mgrid[0:h, 0:w]
    for _ in range(n_rect // 2):
        cx, cy, r = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(2, 7)
        img += float(rng.uniform(-120, 120)) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
    img += rng.normal(0, noise, (h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def check_rotation(extract):
    """The rotation property on `extract(image, **opts) -> dict`: one level, quotas not binding, np.rot90 of the image."""
    img = texture(120, 150, 11)
    H, W = img.shape
    kw = dict(n_levels=1, n_features=5000, fast_threshold=15)
    a, b = extract(img, **kw), extract(np.ascontiguousarray(np.rot90(img)), **kw)
    n = int(a["n_kp"][0])
    assert 20 < n < 2500 and int(b["n_kp"][0]) == n          # (fewer than the stage-1 and stage-2 quotas: not binding)
    # rot90: out[i, j] = img[j, W - 1 - i], so (x, y) -> (y, W - 1 - x)
    mapped = {(int(y), W - 1 - int(x)): k for k, (x, y) in enumerate(a["level_xy"].tolist())}
    assert set(mapped) == {(int(x), int(y)) for x, y in b["level_xy"].tolist()}
    src = np.array([mapped[(int(x), int(y))] for x, y in b["level_xy"].tolist()])
    d = (a["angle"][src].astype(np.float64) - b["angle"].astype(np.float64)) % 360.0
    cs_a, cs_b = a["cs"][src], b["cs"]
    # the direction turns by -90 degrees exactly: (c, s) -> (s, -c)
    assert np.array_equal(cs_b[:, 0], cs_a[:, 1]) and np.array_equal(cs_b[:, 1], -cs_a[:, 0])
    exact = (np.degrees(np.arctan2(cs_a[:, 1], cs_a[:, 0])) - np.degrees(np.arctan2(cs_b[:, 1], cs_b[:, 0]))) % 360.0
    # The 1e-9 degree bound is taken on the fp64 angle of (c, s): the angle OUTPUT is float32, whose spacing near 360 is 3e-5,
    # so it can only be held to 1e-4; the exact (c, s) -> (s, -c) equality above is the stronger statement.
    assert np.abs(exact - 90.0).max() <= 1e-9
    assert np.abs(d - 90.0).max() <= 1e-4                      # (the float32 angles: their spacing at 360 is 3e-5)
    assert np.array_equal(a["desc"][src], b["desc"])
    assert sorted(map(bytes, a["desc"])) == sorted(map(bytes, b["desc"]))
    assert np.array_equal(a["response"][src], b["response"])


EXACT = ("kp_off", "n_kp", "xy", "size", "response", "octave", "level_xy", "cs", "desc")


def assert_equal(got, want):
    """Every output for equality, dtype and shape included; the angle, which goes through atan2, within 1e-4 degrees (float32
    spacing at 360 is 3e-5, plus a few ulp of atan2)."""
    assert set(got) == set(want)
    for k in EXACT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.nonzero(np.asarray(got[k] != want[k]).reshape(len(got[k]), -1).any(axis=1))[0][:8])
    assert got["angle"].dtype == np.float32 and got["angle"].shape == want["angle"].shape
    d = np.abs(got["angle"].astype(np.float64) - want["angle"].astype(np.float64))
    assert (d <= 1e-4).all(), float(d.max())

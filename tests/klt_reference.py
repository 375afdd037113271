"""Yardstick of the KLT tests: a numpy restatement of the definition in include/ba_hip.h (ba_track_klt), one point at a time.
Sums are int64, everything else is float64 with one operation per statement, so each operation is rounded on its own as the
definition asks.  Test infrastructure only; shares no code with the library."""
import numpy as np

OK, OUT, FLAT, FB_FAIL = 0, 1, 2, 3
DEFAULTS = dict(half_window=10, max_level=3, max_iters=30, eps=0.01, min_eig=1e-4, fb_max_px=0.0)
G5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)


def levels(height, width, half_window=10, max_level=3, **_):
    """(level_w, level_h) int32, top level last."""
    n = 2 * half_window + 1
    if min(width, height) < n:
        raise ValueError("the image is smaller than the window")
    ws, hs = [int(width)], [int(height)]
    while len(ws) - 1 < max_level and min((ws[-1] + 1) // 2, (hs[-1] + 1) // 2) >= n:
        ws.append((ws[-1] + 1) // 2)
        hs.append((hs[-1] + 1) // 2)
    return np.array(ws, dtype=np.int32), np.array(hs, dtype=np.int32)


def _reflect(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def down(P):
    """The next pyramid level of a uint8 image."""
    h, w = P.shape
    A = P.astype(np.int64)
    xs = _reflect(2 * np.arange((w + 1) // 2)[:, None] + np.arange(-2, 3)[None], w)        # (wd, 5)
    ys = _reflect(2 * np.arange((h + 1) // 2)[:, None] + np.arange(-2, 3)[None], h)        # (hd, 5)
    rows = (A[:, xs] * G5).sum(axis=2)                                                       # (h, wd)
    out = (rows[ys] * G5[None, :, None]).sum(axis=1)                                         # (hd, wd)
    return ((out + 128) >> 8).astype(np.uint8)


def scharr(P):
    """(Ix, Iy) int64 of a level, coordinates clamped to the image."""
    A = np.pad(P.astype(np.int64), 1, mode="edge")
    Ix = 3 * (A[:-2, 2:] - A[:-2, :-2]) + 10 * (A[1:-1, 2:] - A[1:-1, :-2]) + 3 * (A[2:, 2:] - A[2:, :-2])
    Iy = 3 * (A[2:, :-2] - A[:-2, :-2]) + 10 * (A[2:, 1:-1] - A[:-2, 1:-1]) + 3 * (A[2:, 2:] - A[:-2, 2:])
    return Ix, Iy


def pyramid(img, lw, lh):
    """[(P, Ix, Iy)] per level, all int64."""
    out, P = [], np.ascontiguousarray(img, dtype=np.uint8)
    for l in range(len(lw)):
        if l > 0:
            P = down(P)
        assert P.shape == (int(lh[l]), int(lw[l]))
        out.append((P.astype(np.int64),) + scharr(P))
    return out


def weights(a, b):
    """(w00, w01, w10, w11) of the fractions a (columns) and b (rows): every product rounded, rint half to even."""
    a, b = float(a), float(b)
    ca = 1.0 - a
    cb = 1.0 - b
    t = ca * cb
    w00 = int(np.rint(t * 16384.0))
    t = a * cb
    w01 = int(np.rint(t * 16384.0))
    t = ca * b
    w10 = int(np.rint(t * 16384.0))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def sample(A, cx, cy, n, shift):
    """S(A, c, shift): the n x n window whose top-left corner is c = (cx, cy), int64."""
    fx, fy = float(np.floor(cx)), float(np.floor(cy))
    ix, iy = int(fx), int(fy)
    w00, w01, w10, w11 = weights(cx - fx, cy - fy)
    h, w = A.shape
    xs = np.clip(ix + np.arange(n + 1), 0, w - 1)
    ys = np.clip(iy + np.arange(n + 1), 0, h - 1)
    B = A[np.ix_(ys, xs)]
    v = w00 * B[:-1, :-1] + w01 * B[:-1, 1:] + w10 * B[1:, :-1] + w11 * B[1:, 1:] + (1 << (shift - 1))
    return v >> shift


def inside(x, y, w, h):
    return bool(0.0 <= x and x <= float(w - 1) and 0.0 <= y and y <= float(h - 1))


def track_point(pa, pb, px, py, sx, sy, half_window=10, max_iters=30, eps=0.01, min_eig=1e-4, rec=None, **_):
    """One point from the pyramid pa into pb.  (px, py): the position in a, inside the image; (sx, sy): the start in b, level-0
    pixels.  -> (status, qx, qy, err), err None unless the status is OK.  rec: a list that receives one dict per level visited
    (level, e, iters, exit: eps / osc / cap / out / skipped / flat)."""
    hw, n, L = half_window, 2 * half_window + 1, len(pa) - 1
    px, py = float(px), float(py)
    top = float(1 << L)
    qx, qy = float(sx) / top, float(sy) / top
    eps2 = float(eps) * float(eps)
    T = None
    for l in range(L, -1, -1):
        Pa, Ixa, Iya = pa[l]
        Pb = pb[l][0]
        h, w = Pa.shape
        sc = float(1 << l)
        cx, cy = px / sc - float(hw), py / sc - float(hw)
        T = sample(Pa, cx, cy, n, 9)
        Gx, Gy = sample(Ixa, cx, cy, n, 14), sample(Iya, cx, cy, n, 14)
        A11, A12, A22 = float(int((Gx * Gx).sum())), float(int((Gx * Gy).sum())), float(int((Gy * Gy).sum()))
        t1 = A11 * A22
        t2 = A12 * A12
        D = t1 - t2
        dd = A11 - A22
        dd = dd * dd
        f4 = 4.0 * t2
        root = float(np.sqrt(dd + f4))
        e = (A11 + A22 - root) / float(2 * n * n)
        e = e / 1048576.0
        info = dict(level=l, e=e, iters=0, exit=None)
        if rec is not None:
            rec.append(info)
        if not (D > 0.0) or e < min_eig:
            if l == 0:
                info["exit"] = "flat"
                return FLAT, qx, qy, None
            info["exit"] = "skipped"
            qx, qy = 2.0 * qx, 2.0 * qy
            continue
        info["exit"] = "cap"
        pdx = pdy = 0.0
        for it in range(max_iters):
            if not inside(qx, qy, w, h):
                info["exit"] = "out"
                if l == 0:
                    return OUT, qx, qy, None
                break
            d = sample(Pb, qx - float(hw), qy - float(hw), n, 9) - T
            b1, b2 = float(int((d * Gx).sum())), float(int((d * Gy).sum()))
            u1 = A12 * b2
            u2 = A22 * b1
            dx = (u1 - u2) / D
            u1 = A12 * b1
            u2 = A11 * b2
            dy = (u1 - u2) / D
            qx, qy = qx + dx, qy + dy
            info["iters"] = it + 1
            u1 = dx * dx
            u2 = dy * dy
            if u1 + u2 <= eps2:
                info["exit"] = "eps"
                break
            if it > 0 and abs(dx + pdx) < 0.01 and abs(dy + pdy) < 0.01:
                u1 = 0.5 * dx
                u2 = 0.5 * dy
                qx, qy = qx - u1, qy - u2
                info["exit"] = "osc"
                break
            pdx, pdy = dx, dy
        if l > 0:
            qx, qy = 2.0 * qx, 2.0 * qy
    Pb = pb[0][0]
    h, w = Pb.shape
    if not inside(qx, qy, w, h):
        return OUT, qx, qy, None
    s = int(np.abs(sample(Pb, qx - float(hw), qy - float(hw), n, 9) - T).sum())
    return OK, qx, qy, float(s) / (32.0 * n * n)


def track(images, pairs, points, guess=None, info=None, **opts):
    """ba_track_klt -> dict(pt_off, next, status, err, fb_err, levels) like hip_backend.Solver.track_klt.  images (n, H, W) uint8;
    pairs (n_pairs, 2); points / guess: one (n_p, 2) array per pair.  info: a list that receives, per point in order, the list
    of per-level records of the forward pass (track_point's rec; empty for a point that starts outside)."""
    o = dict(DEFAULTS)
    o.update(opts)
    imgs = np.asarray(images)
    imgs = imgs if imgs.ndim == 3 else imgs[None]
    H, W = imgs.shape[1:]
    lw, lh = levels(H, W, **o)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    pyr = {int(k): pyramid(imgs[int(k)], lw, lh) for k in np.unique(pairs)}
    pts = [np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in points]
    gs = None if guess is None else [np.asarray(g, dtype=np.float32).reshape(-1, 2) for g in guess]
    N = sum(len(p) for p in pts)
    nxt, status = np.zeros((N, 2), np.float32), np.zeros(N, np.uint8)
    err, fb = np.full(N, np.nan, np.float32), np.full(N, np.nan, np.float32)
    k = 0
    for pr, (ia, ib) in enumerate(pairs.tolist()):
        for j in range(len(pts[pr])):
            px, py = float(pts[pr][j, 0]), float(pts[pr][j, 1])
            rec = []
            if info is not None:
                info.append(rec)
            if not inside(px, py, W, H):
                status[k], nxt[k] = OUT, pts[pr][j]
                k += 1
                continue
            sx, sy = (px, py) if gs is None else (float(gs[pr][j, 0]), float(gs[pr][j, 1]))
            st, qx, qy, e = track_point(pyr[ia], pyr[ib], px, py, sx, sy, rec=rec, **o)
            nxt[k] = (np.float32(qx), np.float32(qy))
            if st == OK:
                err[k] = np.float32(e)
                if o["fb_max_px"] > 0:
                    bx, by = float(nxt[k, 0]), float(nxt[k, 1])
                    sb = OUT
                    if inside(bx, by, W, H):
                        sb, rx, ry, _ = track_point(pyr[ib], pyr[ia], bx, by, bx, by, **o)
                    if sb == OK:
                        dx, dy = float(np.float32(rx)) - px, float(np.float32(ry)) - py
                        u1 = dx * dx
                        u2 = dy * dy
                        dist = float(np.sqrt(u1 + u2))
                        fb[k] = np.float32(dist)
                        if dist > o["fb_max_px"]:
                            st = FB_FAIL
                    else:
                        st = FB_FAIL
            status[k] = st
            k += 1
    pt_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
    return dict(pt_off=pt_off, next=nxt, status=status, err=err, fb_err=fb, levels=(lw, lh))


def analytic_image(h, w, dx=0.0, dy=0.0, seed=0, n_waves=60):
    """A sum of n_waves seeded sinusoids with wavelengths 6 .. 60 px, sampled at (x + dx, y + dy), quantised to uint8: the
    content of analytic_image(dx, dy) sits at (x - dx, y - dy) of where analytic_image(0, 0) has it."""
    rng = np.random.default_rng(seed)
    lam = rng.uniform(6.0, 60.0, n_waves)
    th = rng.uniform(0.0, 2.0 * np.pi, n_waves)
    ph = rng.uniform(0.0, 2.0 * np.pi, n_waves)
    amp = rng.uniform(0.5, 1.0, n_waves)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    xx, yy = xx + dx, yy + dy
    v = np.zeros((h, w))
    for k in range(n_waves):
        v += amp[k] * np.sin(2.0 * np.pi / lam[k] * (np.cos(th[k]) * xx + np.sin(th[k]) * yy) + ph[k])
    v = 127.5 + v * (100.0 / np.abs(v).max())
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def assert_equal(got, want):
    """Exact equality of a track_klt result with the yardstick's: next and fb_err bit for bit, err with NaNs in the same places."""
    assert np.array_equal(got["pt_off"], want["pt_off"])
    assert np.array_equal(got["status"], want["status"]), np.nonzero(got["status"] != want["status"])[0][:10]
    for k in ("next", "err", "fb_err"):
        g, w_ = np.asarray(got[k], np.float32), np.asarray(want[k], np.float32)
        assert g.shape == w_.shape and np.array_equal(g.view(np.uint32), w_.view(np.uint32)) or \
            np.array_equal(np.isnan(g), np.isnan(w_)) and np.array_equal(g[~np.isnan(g)], w_[~np.isnan(w_)]), k

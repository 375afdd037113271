"""Host side of shared intrinsics (ba_set_shared_intrinsics): the header, the binding, the group normaliser, the sharding,
the CPU reference the GPU tests compare with, and the generators.  No GPU."""
import ctypes
import hashlib
import os
import re

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.problem import BAProblem, extract_shard, shard_by_landmark
from bundle_adjustment_amd.synthetic import make_bal_problem, make_shared_bal_problem
from tests import robust_losses as rl
from tests import shared_reference as sr
from tests.held_reference import Reduced

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "ba_hip.h")).read()


def test_header_declares_the_function_and_the_stat():
    h = _header()
    assert re.search(r"int\s+ba_set_shared_intrinsics\(ba_handle\*\s*h,\s*const int32_t\*\s*cam_group\);", h)
    stats = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"BA_STAT_(\w+)\s*=\s*(\d+)", h)}
    assert stats["shared_groups"] == 11 and stats["count"] == 10
    assert stats["scratch_bytes"] == 12 and stats["scratch_allocs"] == 13 and stats["end"] == 14      # the scratch arena's two follow it
    assert hip_backend.STATS["shared_groups"] == 11
    assert max(hip_backend.STATS.values()) == stats["end"] - 1
    res, args = hip_backend.SYMBOLS["ba_set_shared_intrinsics"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)]


def test_library_exports_the_symbol():
    lib = ctypes.CDLL(hip_backend.LIB_PATH)
    assert hasattr(lib, "ba_set_shared_intrinsics")


def test_camera_groups_forms():
    cg = hip_backend.camera_groups
    assert cg(None, 5) is None
    assert np.array_equal(cg(True, 4), np.zeros(4, np.int32)) and cg(True, 4).dtype == np.int32
    lab = cg(np.array([3, -1, 3, 7]), 4)
    assert lab.dtype == np.int32 and lab.tolist() == [3, -1, 3, 7]
    assert cg([3, -1, 3, 7], 4).tolist() == [3, -1, 3, 7]
    assert cg([[0, 2], [3]], 5).tolist() == [0, -1, 0, 1, -1]
    assert cg([np.array([4, 1]), []], 5).tolist() == [-1, 0, -1, -1, 0]


@pytest.mark.parametrize("spec,n", [([[0, 5]], 5), ([[-1, 2]], 5), ([[0, 1], [1, 2]], 5), ([[2, 2]], 5), (np.zeros(4, np.int32), 5),
                                    (np.array([0.0, 1.0]), 2), (np.array([True, False]), 2)])
def test_camera_groups_errors(spec, n):
    with pytest.raises(ValueError):
        hip_backend.camera_groups(spec, n)


def test_extract_shard_carries_cam_group():
    bal, lab = make_shared_bal_problem([[0, 2, 4], [1, 3]], 8, 300, 1200, seed=1)
    p = BAProblem(np.ascontiguousarray(bal.cams[:, :6]), bal.pts, bal.cam_idx, bal.pt_idx, bal.uv, np.array([1.0, 1.0, 0.0, 0.0]), -1,
                  cam_group=lab).validate()
    for b, e in shard_by_landmark(p, 2):
        sub, _ = extract_shard(p, b, e)
        assert np.array_equal(sub.cam_group, lab) and sub.cam_group is not lab
    lists = BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, -1, cam_group=[[0, 2, 4], [1, 3]])
    sub, _ = extract_shard(lists, 0, 10)
    assert sub.cam_group == [[0, 2, 4], [1, 3]]
    with pytest.raises(ValueError):
        BAProblem(p.cams, p.pts, p.cam_idx, p.pt_idx, p.uv, p.K4, -1, cam_group=[[0, 99]]).validate()


# ---------------------------------------------------------------------------------- the CPU reference
def _small():
    lab = np.array([4, 9, 4, 9, 4, -1, 7, -1], dtype=np.int32)         # two groups, a singleton (7) and two ungrouped cameras
    bal, lab = make_shared_bal_problem(lab, 8, 200, 900, seed=3)
    mask = np.zeros(8, np.uint16)
    mask[0] = 0x3F
    red = Reduced(bal.cams, bal.pts, bal.cam_idx, bal.pt_idx, bal.uv, None, -1, mask)
    return bal, lab, sr.SharedProblem(red, lab)


def test_expansion_from_labels():
    E = sr.expansion([4, 9, 4, 9, 7], 5, 2).toarray()
    assert E.shape == (5 * 9 + 6, 5 * 9 + 6 - 3 - 3)
    assert (E.sum(axis=1) == 1).all()
    counts = E.sum(axis=0)
    assert sorted(counts[counts > 1].tolist()) == [2.0] * 6                 # two groups of two, three entries each
    x = E @ np.arange(E.shape[1], dtype=np.float64)
    cams = x[:45].reshape(5, 9)
    assert np.array_equal(cams[0, 6:], cams[2, 6:]) and np.array_equal(cams[1, 6:], cams[3, 6:])
    assert not np.array_equal(cams[0, 6:], cams[1, 6:]) and np.unique(cams[:, :6]).size == 30
    assert sr.normalise([4, 9, 4, 7]).tolist() == [4, -1, 4, -1]


def test_shared_gradient_matches_central_differences():
    bal, lab, ref = _small()
    for loss in ("linear", "huber"):
        y = ref.y(bal.cams, bal.pts)
        g = ref.gradient(bal.cams, bal.pts, loss, 2.0)
        assert g.shape == y.shape
        rng = np.random.default_rng(0)
        shared = np.nonzero(np.asarray(ref.E.sum(axis=0)).ravel() > 1)[0]
        assert shared.size == 6
        for j in np.concatenate([shared, rng.integers(0, y.size, 12)]):
            h = 1e-6 * max(1.0, abs(y[j]))
            e = np.zeros_like(y)
            e[j] = h
            fd = (rl.cost(ref.fun(y + e), loss, 2.0) - rl.cost(ref.fun(y - e), loss, 2.0)) / (2 * h)
            assert abs(fd - g[j]) <= 1e-6 * max(abs(g[j]), np.abs(g).max() * 1e-3), (loss, j, fd, g[j])


def test_dense_step_solves_its_system():
    bal, lab, ref = _small()
    lam = 1e-3
    A, g, D = ref.dense_system(bal.cams, bal.pts, "huber", 2.0)
    st = ref.dense_step(bal.cams, bal.pts, lam, "huber", 2.0)
    d = st["step"]
    res = (A + lam * np.diag(D)) @ d + g
    assert np.abs(res).max() <= 1e-9 * np.abs(g).max()
    assert st["model"] > 0 and np.isfinite(st["gain"]) and st["gain"] > 0
    # the trial parameters are x + E d: members of a group stay bit-equal, the held pose does not move
    for m in sr.members(lab).values():
        assert (st["cams"][m, 6:] == st["cams"][m[0], 6:]).all()
    assert np.array_equal(st["cams"][0, :6], bal.cams[0, :6])
    assert np.allclose(ref.step_of(bal.cams, bal.pts, st["cams"], st["pts"]), d, rtol=0, atol=1e-9 * np.abs(d).max())
    # the Marquardt diagonal of a shared entry is the sum of the members' (per-camera) diagonals
    none = sr.SharedProblem(ref.red, -np.ones(8, int))
    Dx = none.dense_system(bal.cams, bal.pts, "huber", 2.0)[2]
    assert np.allclose(D, ref.E.T @ Dx, rtol=1e-15)


# ---------------------------------------------------------------------------------- generators
def test_make_shared_bal_problem_is_deterministic_and_shared():
    a, la = make_shared_bal_problem([[0, 2, 4], [1, 3]], 8, 300, 1200, seed=1, outlier_frac=0.05)
    b, lb = make_shared_bal_problem([[0, 2, 4], [1, 3]], 8, 300, 1200, seed=1, outlier_frac=0.05)
    for x, y in ((a.cams, b.cams), (a.pts, b.pts), (a.uv, b.uv), (a.cam_idx, b.cam_idx), (a.pt_idx, b.pt_idx), (la, lb)):
        assert np.array_equal(x, y)
    assert la.tolist() == [0, 1, 0, 1, 0, -1, -1, -1]
    assert (a.cams[[2, 4], 6:] == a.cams[0, 6:]).all() and (a.cams[3, 6:] == a.cams[1, 6:]).all()
    assert np.unique(a.cams[[0, 1, 5, 6, 7], 6]).size == 5 and (a.cams[:, 8] == 0).all()
    assert np.array_equal(a.uv, a.uv.astype(np.float32).astype(np.float64))
    c, _ = make_shared_bal_problem([[0, 2, 4], [1, 3]], 8, 300, 1200, seed=2)
    assert not np.array_equal(a.uv, c.uv)


def test_make_bal_problem_is_unchanged():
    """Hash of one small output, taken on the commit before shared intrinsics (more than 64 cameras: rotation vectors of
    fewer go through the native walk extension when it is built, with its own last bits)."""
    b = make_bal_problem(70, 300, 1200, seed=1)
    h = hashlib.sha256()
    for a in (b.cams, b.pts, b.cam_idx, b.pt_idx, b.uv):
        h.update(np.ascontiguousarray(a).tobytes())
    assert h.hexdigest() == "bdd1dcd76334e9d923d980253689b0bb95b435a53cc32e5847314387c736a1b3"

"""Launcher of rank processes for the multi-rank tests, and what those tests and their workers share.

launch() starts `world` plain `python worker.py` children that share ONE GPU through the shared-memory transport
(BA_COMM=shm): the 128-byte communicator id is drawn in the parent (ba_comm_unique_id under BA_COMM=shm makes no GPU call)
and travels in the environment, so neither side imports torch.  All children run under one time limit; at the limit every
child is killed and the test fails with the tails of their output.  The parent makes no GPU call while it waits."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 120.0


def unique_id():
    """128 bytes from ba_comm_unique_id under BA_COMM=shm (no GPU call); the caller's BA_COMM is put back."""
    from bundle_adjustment_amd import hip_backend
    old = os.environ.get("BA_COMM")
    os.environ["BA_COMM"] = "shm"
    try:
        return hip_backend.comm_unique_id()
    finally:
        if old is None:
            del os.environ["BA_COMM"]
        else:
            os.environ["BA_COMM"] = old


def _tail(path, n=4000):
    with open(path, "rb") as f:
        f.seek(0, os.SEEK_END)
        f.seek(max(0, f.tell() - n))
        return f.read().decode(errors="replace")


def launch(script, out_dir, world=2, env=None, limit=LIMIT_S):
    """Run `python script` once per rank with RANK, WORLD_SIZE, BA_COMM=shm, BA_COMM_ID (hex) and BA_TEST_OUT (out_dir) in
    the environment and wait for all of them, `limit` seconds at the most.  Every rank's output goes to
    out_dir/rank_<r>.log.  Raises AssertionError naming the ranks that failed -- or, at the limit, after killing every
    child, that the launch hung -- with the tail of every rank's output.  One attempt: nothing is tried again."""
    base = dict(os.environ)
    for k in ("BA_COMM_FORCE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        base.pop(k, None)
    base.update(env or {})
    base.update(BA_COMM="shm", BA_COMM_ID=unique_id().hex(), WORLD_SIZE=str(world), BA_TEST_OUT=str(out_dir), PYTHONUNBUFFERED="1")
    procs, logs = [], []
    for r in range(world):
        logs.append(os.path.join(str(out_dir), f"rank_{r}.log"))
        with open(logs[-1], "wb") as f:
            procs.append(subprocess.Popen([sys.executable, str(script)], env=dict(base, RANK=str(r)), stdout=f, stderr=subprocess.STDOUT,
                                          cwd=ROOT))
    deadline = time.monotonic() + limit
    hung = False
    for p in procs:
        try:
            p.wait(timeout=max(0.0, deadline - time.monotonic()))
        except subprocess.TimeoutExpired:
            hung = True
            break
    if hung:
        for p in procs:
            if p.poll() is None:
                p.kill()
        for p in procs:
            p.wait()
    codes = [p.returncode for p in procs]
    if hung or any(codes):
        tails = "\n".join(f"--- rank {r} (exit {codes[r]}) ---\n{_tail(logs[r])}" for r in range(world))
        raise AssertionError((f"the ranks did not finish within {limit:.0f} s and were killed" if hung else f"rank exit codes {codes}") + "\n" + tails)


# ------------------------------------------------------------------------------------------------ the workers' side
HEADER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
from bundle_adjustment_amd import hip_backend
from tests import multirank as mr
rank, world, OUT = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), os.environ["BA_TEST_OUT"]
uid = bytes.fromhex(os.environ["BA_COMM_ID"])
""" % dict(root=ROOT)


def write_worker(path, body):
    """The worker script: the common header (imports, rank, world, OUT, uid) and the test's body."""
    with open(str(path), "w") as f:
        f.write(HEADER + body)
    return path


def is_bal(prob):
    return prob.cams.shape[1] == 9


def take_points(prob, p_begin, p_end):
    """extract_shard for either camera model: -> (sub-problem of points [p_begin, p_end) with ALL cameras, sel: the positions
    of its observations in the full list)."""
    from bundle_adjustment_amd.bal import BALProblem
    from bundle_adjustment_amd.problem import extract_shard
    if not is_bal(prob):
        return extract_shard(prob, p_begin, p_end)
    sel = np.nonzero((prob.pt_idx >= p_begin) & (prob.pt_idx < p_end))[0]
    return BALProblem(prob.cams.copy(), prob.pts[p_begin:p_end].copy(), prob.cam_idx[sel].copy(),
                      (prob.pt_idx[sel] - p_begin).astype(np.int32), prob.uv[sel].copy()).validate(), sel


def shards(prob, world=2):
    """shard_by_landmark's ranges (they depend on the observation lists alone, which both models share)."""
    from bundle_adjustment_amd.problem import shard_by_landmark
    return shard_by_landmark(prob, world)


def upload(s, prob):
    """The problem onto a handle; -> the (Nc, 3) intrinsics of the BAL camera, None for the pinhole."""
    if is_bal(prob):
        return s.set_problem_bal(prob, 0)
    s.set_problem(prob)
    return None


def residuals(s, intr, loss="huber"):
    """(sse, cost) of the collective residual evaluation in either model."""
    out = s.residuals(loss, want_vector=False) if intr is None else s._residuals_bal_resident(intr, loss, want_vector=False)
    return out[1], out[2]


def flat(prefix, d):
    """A result dict as npz entries `prefix.key` (None entries dropped, scalars as 0-d arrays)."""
    return {f"{prefix}.{k}": np.asarray(v) for k, v in d.items() if v is not None}


def unflat(npz, prefix):
    return {k[len(prefix) + 1:]: npz[k] for k in npz.files if k.startswith(prefix + ".")}


def same_bits(a, b):
    """Two result dicts (or arrays) hold the same bytes: NaN payloads and signed zeros included."""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same_bits(a[k], b[k]) for k in a)
    if a is None or b is None:
        return a is None and b is None
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the problems
K4 = np.array([700.0, 700.0, 640.0, 360.0])
RANSAC_SEED = 7
SIM = (1.7, np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]), np.array([3.0, -2.0, 5.0]))   # s, R (exact 3-4-5 entries), t
_cache = {}


def local_problem(model, share=0.0):
    """make_problem(10, 400, 4) in either camera model (the BAL one with distinct f, k1, k2 per camera): the true points, the
    stock start of the cameras, 0.5 px noise, and a share of uniform mismatches.  Two landmark shards of about 200 points,
    about 80 observations per camera and shard.  -> (problem, true poses, planted (n_obs,) bool)."""
    key = (model, share)
    if key not in _cache:
        from tests import ransac_reference as R
        prob, truth, planted, _ = R.outlier_problem(model, share, seed=41, base=(10, 400, 4))
        _cache[key] = (prob, truth, planted)
    return _cache[key]


def references(prob, seed=3):
    """Reference positions for align: the centres and the points under SIM plus N(0, 0.05).  -> (cam_ref (Nc, 3), pt_ref (Np, 3))."""
    from tests import similarity_reference as sr
    rng = np.random.default_rng(seed)
    s, R, t = SIM
    a = np.concatenate([sr.centres(prob.cams), prob.pts])
    b = s * a @ R.T + t + rng.normal(0.0, 0.05, size=a.shape)
    return b[:prob.n_cams].copy(), b[prob.n_cams:].copy()

"""GPU: shared intrinsics in a multi-rank job -- two ranks on ONE GPU through the shared-memory test transport (BA_COMM=shm),
the recipe of tests/test_gpu_multirank.py::test_two_ranks_bal_camera_match_single_rank.  The group sums run on the
all-reduced product, so both ranks compute the same bits; the in-kernel IPC exchange is not used by grouped solves."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE = dict(loss="huber", max_iters=12, ftol=0.0, xtol=0.0, gtol=0.0, pcg_tol=1e-3, pcg_max_iters=400)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return str(port)


def _input():
    from bundle_adjustment_amd.synthetic import make_shared_bal_problem
    bal, lab = make_shared_bal_problem(np.arange(60) % 3, 60, 5000, 22000, seed=5)      # three interleaved groups of 20
    mask = np.zeros(60, dtype=np.uint16)
    mask[0] = 0x3F                                                                        # the gauge: camera 0's pose
    return bal, lab, mask


WORKER = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, %(root)r)
import torch.distributed as dist
from bundle_adjustment_amd import hip_backend
from bundle_adjustment_amd.problem import BAProblem, extract_shard, shard_by_landmark
from tests.test_gpu_shared_multirank import SOLVE, _input
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group(backend="gloo")
bal, lab, mask = _input()
p = BAProblem(np.ascontiguousarray(bal.cams[:, :6]), bal.pts, bal.cam_idx, bal.pt_idx, bal.uv, np.array([1.0, 1.0, 0.0, 0.0]), -1,
              cam_held=mask, cam_group=lab)
b, e = shard_by_landmark(p, world)[rank]
sub, _ = extract_shard(p, b, e)
s = hip_backend.Solver(0)
uid = [hip_backend.comm_unique_id() if rank == 0 else None]
dist.broadcast_object_list(uid, src=0)
s.comm_init(rank, world, uid[0])
s.set_problem(sub)
intr = np.ascontiguousarray(bal.cams[:, 6:9]).copy()
out = s.solve_bal_resident(intr, **SOLVE)
cams, pts = s.get_params()
np.save(os.path.join(%(out)r, f"cams_{rank}.npy"), np.concatenate([cams, intr], axis=1))
np.save(os.path.join(%(out)r, f"pts_{rank}.npy"), pts)
st = s.stats()
out["ipc_exchanges"], out["shared_groups"] = st["ipc_exchanges"], st["shared_groups"]
json.dump(out, open(os.path.join(%(out)r, f"out_{rank}.json"), "w"))
s.close()
dist.barrier()
dist.destroy_process_group()
"""


@pytest.fixture(scope="module")
def single_rank():
    from bundle_adjustment_amd import hip_backend
    bal, lab, mask = _input()
    with hip_backend.Solver(0) as s:
        return s.solve_bal(bal, held_cameras=mask, shared_intrinsics=lab, **SOLVE)


def _two_ranks(tmp, ipc):
    os.makedirs(tmp, exist_ok=True)
    script = os.path.join(tmp, "worker_shared.py")
    open(script, "w").write(WORKER % dict(root=ROOT, out=str(tmp)))
    env = dict(os.environ, BA_COMM="shm", BA_IPC=ipc)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", _free_port(), script]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    outs = [json.load(open(os.path.join(tmp, f"out_{k}.json"))) for k in range(2)]
    cams = [np.load(os.path.join(tmp, f"cams_{k}.npy")) for k in range(2)]
    pts = np.concatenate([np.load(os.path.join(tmp, f"pts_{k}.npy")) for k in range(2)])
    return outs, cams, pts


def test_two_ranks_shared_intrinsics_match_single_rank(tmp_path, single_rank):
    ref, cams_ref, pts_ref = single_rank
    runs = {ipc: _two_ranks(str(tmp_path / f"ipc{ipc}"), ipc) for ipc in ("0", "1")}
    for ipc, (outs, cams, pts) in runs.items():
        for key in ("iterations", "accepted", "pcg_iterations", "initial_sse", "final_sse", "initial_cost", "final_cost"):
            assert outs[0][key] == outs[1][key], (ipc, key)
        assert outs[0]["shared_groups"] == 3 and outs[1]["shared_groups"] == 3
        assert outs[0]["ipc_exchanges"] == 0 and outs[1]["ipc_exchanges"] == 0            # the base transport serves grouped solves
        assert np.array_equal(cams[0], cams[1]) and cams[0].shape == (60, 9)
        for g in range(3):
            m = np.arange(g, 60, 3)
            assert (cams[0][m, 6:].view(np.uint64) == cams[0][m[0], 6:].view(np.uint64)).all()
            assert not np.array_equal(cams[0][m[0], 6:], _input()[0].cams[m[0], 6:])
        assert abs(outs[0]["initial_cost"] - ref["initial_cost"]) <= 1e-10 * ref["initial_cost"]
        assert abs(outs[0]["final_cost"] - ref["final_cost"]) <= 1e-8 * ref["final_cost"]
        assert outs[0]["final_cost"] < outs[0]["initial_cost"]
        assert np.abs(cams[0] - cams_ref).max() <= 1e-6 * np.abs(cams_ref).max()
        assert pts.shape == pts_ref.shape and np.abs(pts - pts_ref).max() <= 1e-5 * np.abs(pts_ref).max()
    # BA_IPC=1 changes nothing for a grouped solve
    for a, b in zip(runs["0"][0], runs["1"][0]):
        assert {k: v for k, v in a.items() if not k.startswith("seconds")} == {k: v for k, v in b.items() if not k.startswith("seconds")}
    assert np.array_equal(runs["0"][1][0], runs["1"][1][0]) and np.array_equal(runs["0"][2], runs["1"][2])

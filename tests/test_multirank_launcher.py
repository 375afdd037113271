"""CPU: the rank launcher of the multi-rank GPU tests (tests/multirank.py) -- what its children find in their environment,
how a failing rank is reported, and the helpers that carry results between the processes.  No GPU call on either side."""
import json
import os

import numpy as np
import pytest

from tests import multirank as mr

ECHO = r"""
json.dump(dict(rank=rank, world=world, uid=uid.hex(), comm=os.environ["BA_COMM"], forced="BA_COMM_FORCE" in os.environ,
               extra=os.environ.get("EXTRA")), open(os.path.join(OUT, f"echo_{rank}.json"), "w"))
"""


def test_children_get_rank_world_transport_and_one_id(tmp_path, monkeypatch):
    import __graft_entry__ as g
    g.build()
    monkeypatch.setenv("BA_COMM_FORCE", "1")                 # a forced one-rank communicator of the parent must not leak
    monkeypatch.delenv("BA_COMM", raising=False)
    mr.launch(mr.write_worker(tmp_path / "worker.py", ECHO), tmp_path, world=3, env=dict(EXTRA="x"))
    got = [json.load(open(tmp_path / f"echo_{r}.json")) for r in range(3)]
    assert [g_["rank"] for g_ in got] == [0, 1, 2] and all(g_["world"] == 3 and g_["comm"] == "shm" and not g_["forced"] for g_ in got)
    assert len(bytes.fromhex(got[0]["uid"])) == 128 and got[0]["uid"] == got[1]["uid"] == got[2]["uid"] and got[0]["extra"] == "x"
    assert "BA_COMM" not in os.environ                       # the parent's own transport choice is put back
    assert mr.unique_id() != bytes.fromhex(got[0]["uid"])    # another launch, another id


def test_a_failing_rank_fails_the_launch_with_every_ranks_tail(tmp_path):
    import __graft_entry__ as g
    g.build()
    body = "print('rank', rank, 'was here')\nif rank == 1:\n    raise SystemExit(3)\n"
    with pytest.raises(AssertionError) as err:
        mr.launch(mr.write_worker(tmp_path / "worker.py", body), tmp_path)
    msg = str(err.value)
    assert "rank exit codes [0, 3]" in msg and "rank 0 was here" in msg and "rank 1 was here" in msg


def test_results_travel_as_npz_and_compare_by_bits(tmp_path):
    res = dict(poses=np.arange(12.0).reshape(2, 6), status=np.array([0, 1], dtype=np.uint8), rms=np.float64("nan"), none=None)
    np.savez(tmp_path / "r.npz", **mr.flat("comm.resect", res), **mr.flat("comm.ransac", dict(poses=np.zeros(3))))
    back = mr.unflat(np.load(tmp_path / "r.npz"), "comm.resect")
    assert set(back) == {"poses", "status", "rms"} and mr.same_bits(back, {k: v for k, v in res.items() if v is not None})
    assert mr.same_bits(np.array([np.nan]), np.array([np.nan])) and not mr.same_bits(np.array([0.0]), np.array([-0.0]))
    assert not mr.same_bits(np.zeros(2), np.zeros(3)) and not mr.same_bits(np.zeros(2), np.zeros(2, dtype=np.float32))
    assert not mr.same_bits(dict(a=np.zeros(1)), dict(b=np.zeros(1)))


def test_the_shards_of_both_camera_models_are_the_same_observations():
    pin, bal = mr.local_problem("pinhole", 0.3), mr.local_problem("bal", 0.3)
    assert mr.is_bal(bal[0]) and not mr.is_bal(pin[0]) and mr.shards(pin[0]) == mr.shards(bal[0]) == [(0, 200), (200, 400)]
    seen = np.zeros(pin[0].n_obs, dtype=int)
    for b, e in mr.shards(pin[0]):
        (sp, sel_p), (sb, sel_b) = mr.take_points(pin[0], b, e), mr.take_points(bal[0], b, e)
        assert np.array_equal(sel_p, sel_b) and np.array_equal(sp.pt_idx, sb.pt_idx) and np.array_equal(sp.cam_idx, sb.cam_idx)
        assert sp.n_pts == sb.n_pts == e - b and sb.cams.shape == (10, 9) and np.array_equal(sb.uv, bal[0].uv[sel_b])
        assert np.bincount(sp.cam_idx, minlength=10).min() >= 65          # more than a wave per camera and shard
        seen[sel_p] += 1
    assert (seen == 1).all()

"""GPU: the rank-local calls -- ba_triangulate_tracks, ba_resect, ba_resect_ransac, ba_transform, ba_align, ba_get_centres --
on handles that carry a communicator.  (a) a forced communicator of one rank against a plain handle, bit for bit; (b) two
ranks sharing one GPU (shm transport, tests/multirank.py): each rank's shard against a plain handle on the same shard in the
same process, and against the numpy yardsticks of the single-rank tests run on the SUB-problem, with their tolerances -- a
camera on rank r is resected from the shard's observations; (c) no collective inside: one rank alone makes the calls and the
next collective still meets; (d) the state after the writes that are legitimate on several ranks, and a solve from it;
(e) a rank without landmarks; (f) the writes that would split the replicated cameras are refused when world > 1."""
import functools
import json

import numpy as np
import pytest

from bundle_adjustment_amd import hip_backend
from tests import multirank as mr
from tests import ransac_reference as R
from tests import resect_reference as rr
from tests import similarity_reference as sr
from tests import track_reference as tr
from tests.multirank import same_bits
from tests.resect_reference import pose_diff
from tests.test_gpu_ransac import THR, errors
from tests.test_gpu_similarity import compare_alignment
from tests.test_gpu_tracks import OPTS, check_measures, decided_far_from_threshold, parity_problem, parity_reference, _rel

pytestmark = pytest.mark.gpu
MODELS = ["pinhole", "bal"]
FEW_POINTS, TOO_FEW = hip_backend.RESECT_STATUS["few_points"], hip_backend.ALIGN_STATUS["too_few"]
SOLVE = dict(loss="huber", max_iters=10, pcg_tol=1e-3)


def solve(s, intr, **kw):
    return s.solve(**kw) if intr is None else s.solve_bal_resident(intr, **kw)


def load(tmp, name, world=2):
    return [np.load(tmp / f"{name}_{r}.npz") for r in range(world)]


def alignment(d):
    """A saved align result as Solver.align returns it (scalars as numbers, the absent error array as None)."""
    out = {k: (v.item() if v.ndim == 0 else v) for k, v in d.items()}
    out.setdefault("cam_err", None)
    out.setdefault("pt_err", None)
    return out


# ------------------------------------------------------------------------------------------------ (a) forced, in process
def every_call(s, model):
    """The five calls and centres() on handle s, both losses, write_* / apply 0 and 1: -> list of (label, result)."""
    clean, dirty, tracks = mr.local_problem(model)[0], mr.local_problem(model, 0.3)[0], parity_problem(model)[0]
    cam_ref, pt_ref = mr.references(clean)
    got = []

    def state(label, intr):
        cams, pts = s.get_params()
        got.append((label + " params", dict(cams=cams, pts=pts, sse=np.float64(mr.residuals(s, intr)[0]))))

    intr = mr.upload(s, clean)
    got.append(("clean scalars", s.debug_layout("scalars")))
    got.append(("centres", s.centres()))
    for loss in ("linear", "huber"):
        got.append((f"resect {loss}", s.resect(intr=intr, loss=loss)))
        got.append((f"align cameras {loss}", s.align(cam_ref=cam_ref, loss=loss, f_scale=0.15)))
        got.append((f"align points {loss}", s.align(pt_ref=pt_ref, loss=loss, f_scale=0.15)))
    got.append(("resect write", s.resect(intr=intr, loss="huber", write_cams=1)))
    state("resect write", intr)
    s.transform(*mr.SIM)
    state("transform", intr)
    got.append(("align apply", s.align(cam_ref=cam_ref, pt_ref=pt_ref, loss="huber", f_scale=0.15, apply=True)))
    state("align apply", intr)
    got.append(("centres after", s.centres()))
    intr = mr.upload(s, dirty)
    for loss in ("linear", "huber"):
        got.append((f"ransac {loss}", s.resect_ransac(intr=intr, loss=loss, seed=mr.RANSAC_SEED)))
    got.append(("ransac write", s.resect_ransac(intr=intr, seed=mr.RANSAC_SEED, write_cams=1)))
    state("ransac write", intr)
    intr = mr.upload(s, tracks)
    got.append(("tracks scalars", s.debug_layout("scalars")))
    for loss in ("linear", "huber"):
        got.append((f"tracks {loss}", s.triangulate_tracks(intr=intr, loss=loss, **OPTS)))
    got.append(("tracks write", s.triangulate_tracks(intr=intr, write_points=1, **OPTS)))
    state("tracks write", intr)
    return got


@pytest.mark.parametrize("model", MODELS)
def test_forced_one_rank_communicator_gives_the_plain_handles_bits(model, monkeypatch):
    """BA_COMM_FORCE=1 puts a handle on the multi-rank control flow without a second process (world == 1: no write is
    refused).  Same kernels, same data, fixed-order sums: every returned array, the layout scalars, and after every write
    get_params and the sse of residuals() are the plain handle's, bit for bit."""
    with hip_backend.Solver(0) as s:
        plain = every_call(s, model)
    monkeypatch.setenv("BA_COMM", "shm")
    monkeypatch.setenv("BA_COMM_FORCE", "1")
    with hip_backend.Solver(0) as s:
        s.comm_init(0, 1, hip_backend.comm_unique_id())
        forced = every_call(s, model)
    assert [k for k, _ in plain] == [k for k, _ in forced]
    for (label, a), (_, b) in zip(plain, forced):
        if label.endswith("scalars"):
            assert a == b, label
        else:
            assert same_bits(a, b), label
    done = dict(plain)
    assert (done["resect write"]["status"] == rr.OK).all() and (done["ransac write"]["status"] == R.OK).all()
    assert done["align apply"]["status"] == 0 and not same_bits(done["centres"], done["centres after"])


# ------------------------------------------------------------------------------------------------ (b) two ranks, per shard
SHARD_WORKER = r"""
from tests.test_gpu_tracks import OPTS, parity_problem
model = os.environ["MODEL"]
clean, dirty, tracks = mr.local_problem(model)[0], mr.local_problem(model, 0.3)[0], parity_problem(model)[0]
cam_ref, pt_ref = mr.references(clean)
comm, plain = hip_backend.Solver(0), hip_backend.Solver(0)
comm.comm_init(rank, world, uid)
out = {}
for name, s in (("comm", comm), ("plain", plain)):
    b, e = mr.shards(clean)[rank]
    intr = mr.upload(s, mr.take_points(clean, b, e)[0])
    out.update(mr.flat(name + ".resect", s.resect(intr=intr)))
    out.update(mr.flat(name + ".align_cams", s.align(cam_ref=cam_ref)))
    out.update(mr.flat(name + ".align_pts", s.align(pt_ref=pt_ref[b:e])))
    out[name + ".centres"] = s.centres()
    intr = mr.upload(s, mr.take_points(dirty, b, e)[0])
    out.update(mr.flat(name + ".ransac", s.resect_ransac(intr=intr, seed=mr.RANSAC_SEED)))
    b, e = mr.shards(tracks)[rank]
    for lanes in ("", "2"):            # 2 lanes per point: the library then splits off the long tracks (read by ba_set_problem)
        if lanes:
            os.environ["BA_PT_LANES"] = lanes
        intr = mr.upload(s, mr.take_points(tracks, b, e)[0])
        os.environ.pop("BA_PT_LANES", None)
        out.update(mr.flat(name + ".tracks" + lanes, s.triangulate_tracks(intr=intr, **OPTS)))
        out[name + ".long" + lanes] = np.array(s.debug_layout("scalars")["n_long"])
np.savez(os.path.join(OUT, f"shard_{rank}.npz"), **out)
comm.close()
plain.close()
"""
CALLS = ("resect", "align_cams", "align_pts", "ransac", "tracks", "tracks2")


@pytest.fixture(scope="module", params=MODELS)
def shard_run(request, tmp_path_factory):
    """One launch per camera model: -> (model, the two ranks' saved results)."""
    tmp = tmp_path_factory.mktemp("shards_" + request.param)
    mr.launch(mr.write_worker(tmp / "worker.py", SHARD_WORKER), tmp, env=dict(MODEL=request.param))
    return request.param, load(tmp, "shard")


def test_a_communicator_handle_gives_the_plain_handles_bits_on_its_shard(shard_run):
    model, got = shard_run
    for r in range(2):
        for call in CALLS:
            assert same_bits(mr.unflat(got[r], "comm." + call), mr.unflat(got[r], "plain." + call)), (r, call)
        assert same_bits(got[r]["comm.centres"], got[r]["plain.centres"])
    # the cameras are replicated: what depends on them alone is the same on both ranks
    assert same_bits(mr.unflat(got[0], "comm.align_cams"), mr.unflat(got[1], "comm.align_cams"))
    assert same_bits(got[0]["comm.centres"], got[1]["comm.centres"])
    assert not same_bits(got[0]["comm.resect.poses"], got[1]["comm.resect.poses"])       # (each from its shard's observations)


def test_resect_on_a_shard_is_the_yardsticks_resection_of_the_sub_problem(shard_run):
    """test_gpu_resect's checks on each rank's sub-problem: status and inlier counts, poses within 10 d_ref + 1e-12 (d_ref: the
    yardstick from its DLT against the yardstick from the true poses), the measures those of the yardstick at the device's pose."""
    model, got = shard_run
    prob, truth, _ = mr.local_problem(model)
    for r, (b, e) in enumerate(mr.shards(prob)):
        sub, _ = mr.take_points(prob, b, e)
        out = mr.unflat(got[r], "comm.resect")
        ref, from_truth = rr.resect_cameras(sub), rr.resect_cameras(sub, x0=truth)
        assert (ref["status"] == rr.OK).all() and np.bincount(sub.cam_idx, minlength=10).min() >= 65       # the fixture: more than a wave each
        d_ref = float(pose_diff(ref["poses"], from_truth["poses"]).max())
        d = pose_diff(out["poses"], ref["poses"])
        print(f"{model} rank {r}: d_ref {d_ref:.3e}, device against the reference {d.max():.3e}")
        assert np.array_equal(out["status"], ref["status"]) and np.array_equal(out["n_inliers"], ref["n_inliers"])
        assert np.array_equal(out["n_inliers"], np.bincount(sub.cam_idx, minlength=10))
        assert d.max() <= 10.0 * d_ref + 1e-12
        for c in range(sub.n_cams):
            m = rr.resect(rr.obs_of(sub, c), out["poses"][c], init="current", refine_iters=0)
            assert m["n_inliers"] == out["n_inliers"][c]
            assert abs(out["rms_px"][c] - m["rms_px"]) <= 1e-9 * m["rms_px"] and abs(out["max_px"][c] - m["max_px"]) <= 1e-9 * m["max_px"]


def test_ransac_on_a_shard_and_its_mask_in_the_callers_observation_order(shard_run):
    """test_gpu_ransac's outcome check on each rank's sub-problem (30 % uniform mismatches): consensus = the yardstick's
    inliers, poses within 10 d_ref + 1e-12 of the yardstick (d_ref: the reference's own RANSAC + LO against it).  obs_inlier
    scattered through extract_shard's sel is a mask over the caller's full observation list."""
    model, got = shard_run
    prob, truth, planted = mr.local_problem(model, 0.3)
    full, want = np.zeros(prob.n_obs, dtype=bool), np.zeros(prob.n_obs, dtype=bool)
    seen = np.zeros(prob.n_obs, dtype=int)
    for r, (b, e) in enumerate(mr.shards(prob)):
        sub, sel = mr.take_points(prob, b, e)
        out = mr.unflat(got[r], "comm.ransac")
        yard = R.yardstick_poses(sub, truth, planted[sel])
        err, depth = errors(sub, yard)
        assert (np.abs(err - THR) > 1e-6).all() and (depth > 0.0).all()          # the fixture: no observation sits on the threshold
        ref = R.resect_ransac(sub, n_hyp=256, seed=mr.RANSAC_SEED)
        assert (ref["status"] == R.OK).all()
        d_ref = float(pose_diff(ref["poses"], yard).max())
        d = pose_diff(out["poses"], yard)
        print(f"{model} rank {r}: d_ref {d_ref:.3e}, device against the yardstick {d.max():.3e}")
        assert (out["status"] == R.OK).all()
        assert out["obs_inlier"].shape == (sub.n_obs,) and np.array_equal(out["obs_inlier"], err <= THR)
        assert np.array_equal(out["n_inliers"], np.bincount(sub.cam_idx[out["obs_inlier"]], minlength=sub.n_cams))
        assert d.max() <= 10.0 * d_ref + 1e-12
        full[sel], want[sel] = out["obs_inlier"], err <= THR
        seen[sel] += 1
    assert (seen == 1).all()                                                 # the shards' observations partition the caller's list
    assert np.array_equal(full, want) and np.array_equal(full, ~planted)      # (the consensus is the planted inliers)


def test_align_and_centres_on_a_shard_match_the_yardstick(shard_run):
    """test_gpu_similarity's parity bound (1e-10 on s, R, t and the errors) for cam_ref alone and for pt_ref alone, the
    latter over the shard's points; centres to 1e-13 x 20 as there."""
    model, got = shard_run
    prob = mr.local_problem(model)[0]
    cam_ref, pt_ref = mr.references(prob)
    t_scale = max(1.0, float(np.linalg.norm(mr.SIM[2])))
    ctr = sr.centres(prob.cams)
    sims = []
    for r, (b, e) in enumerate(mr.shards(prob)):
        assert np.abs(got[r]["comm.centres"] - ctr).max() <= 1e-13 * 20
        d_c = compare_alignment(alignment(mr.unflat(got[r], "comm.align_cams")), sr.align(ctr, cam_ref), t_scale)
        pts = alignment(mr.unflat(got[r], "comm.align_pts"))
        d_p = compare_alignment(pts, sr.align(prob.pts[b:e], pt_ref[b:e]), t_scale)
        print(f"{model} rank {r}: align cameras {np.array2string(d_c, precision=2)}, points {np.array2string(d_p, precision=2)}")
        assert (d_c <= 1e-10).all() and (d_p <= 1e-10).all()
        assert pts["n_used"] == e - b and pts["pt_err"].shape == (e - b,)
        sims.append(pts["t"])
    assert not same_bits(sims[0], sims[1])                                    # (the points differ from rank to rank, and so does the estimate)


def test_tracks_on_a_shard_match_the_yardstick_and_the_whole_problems_statuses(shard_run):
    """test_gpu_tracks' checks on each rank's sub-problem (the long tracks and the special points 240-251 are in the second
    shard): statuses, points within 10 d_ref + 1e-12 (d_ref: the yardstick from its DLT against the yardstick from the true
    point), measures.  The two shards' statuses, concatenated, are the single-rank statuses of the whole problem."""
    model, got = shard_run
    prob, truth = parity_problem(model)
    ranges = mr.shards(prob)
    assert ranges[0][1] <= 240 and ranges[1][1] == prob.n_pts
    for r, (b, e) in enumerate(ranges):
        sub, _ = mr.take_points(prob, b, e)
        ref = tr.triangulate_tracks(sub, **OPTS)
        far = decided_far_from_threshold(ref, OPTS)
        ok = np.isfinite(ref["xyz"]).all(axis=1)
        other = tr.triangulate_tracks(sub, points=np.nonzero(ok)[0], refine_iters=20, x0=truth[b:e], **OPTS)
        d_ref = float(_rel(other["xyz"], ref["xyz"][ok]).max())
        for form in ("tracks", "tracks2"):                   # one launch form, and the long tracks split off
            out = mr.unflat(got[r], "comm." + form)
            n_long = int(got[r]["comm.long" + form[6:]])
            assert far.all() and out["status"].shape == (e - b,)
            assert np.array_equal(out["status"][far], ref["status"][far])
            dev = float(_rel(out["xyz"][ok], ref["xyz"][ok]).max())
            print(f"{model} rank {r}: d_ref {d_ref:.3e}, device against the reference {dev:.3e}; long tracks split off: {n_long}")
            assert dev <= 10.0 * d_ref + 1e-12
            assert np.array_equal(np.isfinite(out["xyz"]).all(axis=1), ok)
            check_measures(sub, out, np.nonzero(ok)[0])
            # the tracks of 65, 70 and 130 views are long whatever threshold the shard's own statistic sets
            assert n_long == 0 if form == "tracks" or r == 0 else n_long >= 3
    assert set(mr.unflat(got[1], "comm.tracks")["status"]) == set(range(6))    # every status occurs in the second shard
    whole_ref = parity_reference(model, "linear", 20)
    far = decided_far_from_threshold(whole_ref, OPTS)
    with hip_backend.Solver(0) as s:
        whole = s.triangulate_tracks(intr=mr.upload(s, prob), **OPTS)
    assert far.sum() >= 0.99 * prob.n_pts
    for form in ("tracks", "tracks2"):
        both = np.concatenate([got[r][f"comm.{form}.status"] for r in range(2)])
        assert both.shape == whole["status"].shape
        assert np.array_equal(both[far], whole["status"][far]) and np.array_equal(both[far], whole_ref["status"][far])


# ------------------------------------------------------------------------------------------------ (c) no collective
ALONE_WORKER = r"""
from tests.test_gpu_tracks import OPTS
model = os.environ["MODEL"]
prob = mr.local_problem(model)[0]
cam_ref, pt_ref = mr.references(prob)
b, e = mr.shards(prob)[rank]
s = hip_backend.Solver(0)
s.comm_init(rank, world, uid)
intr = mr.upload(s, mr.take_points(prob, b, e)[0])
calls = 0
if rank == 0:                      # rank 1 makes none of them
    s.triangulate_tracks(intr=intr, **OPTS); s.resect(intr=intr); s.resect_ransac(intr=intr, seed=mr.RANSAC_SEED)
    s.align(cam_ref=cam_ref); s.align(pt_ref=pt_ref[b:e]); s.centres()
    s.transform(1.0, np.eye(3), np.zeros(3))           # (the identity: the parameters keep their values, set 0 becomes current)
    calls = 7
sse, cost = mr.residuals(s, intr, "huber")              # the collective both ranks must meet in
json.dump(dict(sse=sse, cost=cost, calls=calls), open(os.path.join(OUT, f"alone_{rank}.json"), "w"))
s.close()
"""


def whole_problem_sse(prob, prepare=None):
    with hip_backend.Solver(0) as s:
        intr = mr.upload(s, prob)
        if prepare:
            prepare(s)
        return mr.residuals(s, intr, "huber")


@pytest.mark.parametrize("model", MODELS)
def test_the_calls_hold_no_collective(model, tmp_path):
    """Rank 0 alone makes the five calls (nothing written but the identity transform) and centres(); rank 1 makes none.  The
    collective residuals() that follows returns on both ranks with the single-rank sse of the whole problem to 1e-10."""
    mr.launch(mr.write_worker(tmp_path / "worker.py", ALONE_WORKER), tmp_path, env=dict(MODEL=model))
    got = [json.load(open(tmp_path / f"alone_{r}.json")) for r in range(2)]
    assert got[0]["calls"] == 7 and got[1]["calls"] == 0
    sse, cost = whole_problem_sse(mr.local_problem(model)[0])
    assert got[0]["sse"] == got[1]["sse"] and got[0]["cost"] == got[1]["cost"]
    assert abs(got[0]["sse"] - sse) <= 1e-10 * sse and abs(got[0]["cost"] - cost) <= 1e-10 * cost


# ------------------------------------------------------------------------------------------------ (d) the legitimate writes
def legitimate_writes(s, intr, cam_ref):
    """triangulate_tracks(write_points=1), the same similarity on every rank, align on the cameras alone and applied."""
    trk = s.triangulate_tracks(intr=intr, write_points=1)
    s.transform(*mr.SIM)
    return trk, s.align(cam_ref=cam_ref, apply=True)


WRITE_WORKER = r"""
from tests.test_gpu_multirank_local import SOLVE, legitimate_writes, solve
model = os.environ["MODEL"]
prob = mr.local_problem(model)[0]
cam_ref, _ = mr.references(prob)
b, e = mr.shards(prob)[rank]
s = hip_backend.Solver(0)
s.comm_init(rank, world, uid)
intr = mr.upload(s, mr.take_points(prob, b, e)[0])
trk, al = legitimate_writes(s, intr, cam_ref)
cams, pts = s.get_params()
summary = solve(s, intr, **SOLVE)
cams2, pts2 = s.get_params()
extra = {} if intr is None else dict(intr=intr)
np.savez(os.path.join(OUT, f"write_{rank}.npz"), cams=cams, pts=pts, cams2=cams2, pts2=pts2, status=trk["status"], **extra, **mr.flat("align", al))
json.dump(summary, open(os.path.join(OUT, f"write_{rank}.json"), "w"))
s.close()
"""


@functools.lru_cache(maxsize=None)
def track_spread(model):
    """d_ref of test_gpu_tracks on the whole problem: the yardstick from its DLT against the yardstick from the true point."""
    prob = mr.local_problem(model)[0]             # (its points ARE the true ones)
    ref = tr.triangulate_tracks(prob)
    other = tr.triangulate_tracks(prob, x0=prob.pts)
    assert np.isfinite(ref["xyz"]).all() and (ref["status"] == tr.OK).all()
    return float(_rel(other["xyz"], ref["xyz"]).max())


@pytest.mark.parametrize("model", MODELS)
def test_state_after_the_legitimate_writes_and_a_solve_from_it(model, tmp_path):
    """Points are rank-local, so write_points = 1 is legitimate on every rank; so is ba_transform with the same similarity
    and ba_align on the cameras alone.  Afterwards the cameras are the same bits on both ranks and on a single-rank handle
    that made the same calls on the whole problem (they are replicated, and nothing that moved them saw a point); the
    concatenated points are the single-rank handle's within what the single-rank tests allow: both sides lie within
    10 d_ref + 1e-12 (relative, per point) of the yardstick's triangulation, the two similarities scale that by s s', and
    each of the two transforms may add 1e-13 of the largest coordinate.  A solve from there agrees with the single-rank
    solve in the bounds of test_two_ranks_on_one_gpu_match_single_rank: 1e-9 relative cost, cameras 1e-6, points 1e-5."""
    prob = mr.local_problem(model)[0]
    cam_ref, _ = mr.references(prob)
    mr.launch(mr.write_worker(tmp_path / "worker.py", WRITE_WORKER), tmp_path, env=dict(MODEL=model))
    got = load(tmp_path, "write")
    outs = [json.load(open(tmp_path / f"write_{r}.json")) for r in range(2)]
    with hip_backend.Solver(0) as s:
        intr = mr.upload(s, prob)
        before = s.get_params()[1]
        trk, al = legitimate_writes(s, intr, cam_ref)
        cams, pts = s.get_params()
        ref = solve(s, intr, **SOLVE)
        cams2, pts2 = s.get_params()
    assert (trk["status"] == tr.OK).all() and al["status"] == 0 and not np.array_equal(before, pts)
    assert same_bits(got[0]["cams"], got[1]["cams"]) and same_bits(got[0]["cams"], cams)
    assert same_bits(mr.unflat(got[0], "align"), mr.unflat(got[1], "align"))
    assert same_bits(alignment(mr.unflat(got[0], "align"))["R"], al["R"]) and alignment(mr.unflat(got[0], "align"))["s"] == al["s"]
    both = np.concatenate([got[r]["pts"] for r in range(2)])
    assert both.shape == pts.shape and np.array_equal(np.concatenate([got[r]["status"] for r in range(2)]), trk["status"])
    s_total = mr.SIM[0] * al["s"]
    x_before = np.abs((pts - al["t"]) @ al["R"] / al["s"] - mr.SIM[2]).max(axis=1) / mr.SIM[0]      # |X| of the triangulated point, largest coordinate (R is orthogonal: bounded by sqrt(3) below)
    bound = 2.0 * s_total * 3.0 * (10.0 * track_spread(model) + 1e-12) * x_before + 4e-13 * max(1.0, float(np.abs(pts).max()))
    d = np.abs(both - pts).max(axis=1)
    print(f"{model}: points after the writes, two ranks against one: largest difference {d.max():.3e}, largest share of its bound {(d / bound).max():.3e}")
    assert (d <= bound).all()
    for key in ("iterations", "accepted", "pcg_iterations", "initial_sse", "final_sse", "initial_cost", "final_cost", "status"):
        assert outs[0][key] == outs[1][key], key
    print(f"{model}: solve {outs[0]['iterations']} iterations, cost {outs[0]['initial_cost']:.6f} -> {outs[0]['final_cost']:.6f} (one rank {ref['final_cost']:.6f}), "
          f"cameras {np.abs(got[0]['cams2'] - cams2).max():.3e}, points {np.abs(np.concatenate([got[r]['pts2'] for r in range(2)]) - pts2).max():.3e}")
    assert outs[0]["iterations"] >= 2 and outs[0]["final_cost"] < outs[0]["initial_cost"]
    assert abs(outs[0]["initial_sse"] - ref["initial_sse"]) <= 1e-10 * ref["initial_sse"]
    assert abs(outs[0]["final_cost"] - ref["final_cost"]) <= 1e-9 * ref["final_cost"]
    assert same_bits(got[0]["cams2"], got[1]["cams2"]) and np.abs(got[0]["cams2"] - cams2).max() <= 1e-6
    assert np.abs(np.concatenate([got[r]["pts2"] for r in range(2)]) - pts2).max() <= 1e-5
    if intr is not None:
        assert same_bits(got[0]["intr"], got[1]["intr"]) and np.abs(got[0]["intr"] - intr).max() <= 1e-6 * np.abs(intr).max()


# ------------------------------------------------------------------------------------------------ (e) the empty shard
EMPTY_WORKER = r"""
from tests.test_gpu_tracks import OPTS
prob = mr.local_problem("pinhole")[0]
cam_ref, pt_ref = mr.references(prob)
b, e = (0, prob.n_pts) if rank == 0 else (prob.n_pts, prob.n_pts)          # rank 1 owns no landmark at all
s = hip_backend.Solver(0)
s.comm_init(rank, world, uid)
intr = mr.upload(s, mr.take_points(prob, b, e)[0])
out = {}
out.update(mr.flat("tracks", s.triangulate_tracks(**OPTS)))
out.update(mr.flat("resect", s.resect()))
out.update(mr.flat("ransac", s.resect_ransac(seed=mr.RANSAC_SEED)))
out.update(mr.flat("align_pts", s.align(pt_ref=pt_ref[b:e])))
out.update(mr.flat("align_cams", s.align(cam_ref=cam_ref)))
out["centres"] = s.centres()
s.triangulate_tracks(write_points=1, want=False)
s.transform(*mr.SIM)
out["sse"] = np.array(mr.residuals(s, intr, "huber"))
np.savez(os.path.join(OUT, f"empty_{rank}.npz"), **out)
s.close()
"""


def test_a_rank_without_landmarks_makes_every_call(tmp_path):
    """Rank 1 owns no landmark: every call returns BA_OK (the worker would exit non-zero otherwise) -- triangulate_tracks
    arrays of length 0, every camera FEW_POINTS for both resections, align(pt_ref = empty) TOO_FEW -- and the collective
    residuals() after the legitimate writes is the single-rank handle's after the same writes."""
    mr.launch(mr.write_worker(tmp_path / "worker.py", EMPTY_WORKER), tmp_path)
    got = load(tmp_path, "empty")
    prob = mr.local_problem("pinhole")[0]
    e = got[1]
    for key in ("xyz", "status", "angle_deg", "rms_px", "max_px"):
        assert e["tracks." + key].shape[0] == 0 and got[0]["tracks." + key].shape[0] == prob.n_pts
    for call in ("resect", "ransac"):
        assert (e[call + ".status"] == FEW_POINTS).all() and e[call + ".status"].shape == (prob.n_cams,)
        assert np.array_equal(e[call + ".poses"], prob.cams[:, :6]) and (e[call + ".n_inliers"] == 0).all()
        assert np.isnan(e[call + ".rms_px"]).all() and np.isnan(e[call + ".max_px"]).all()
        assert (got[0][call + ".status"] == rr.OK).all()
    assert e["ransac.obs_inlier"].shape == (0,)
    assert e["align_pts.status"] == TOO_FEW and e["align_pts.n_used"] == 0 and e["align_pts.pt_err"].shape == (0,)
    assert got[0]["align_pts.status"] == 0 and got[0]["align_pts.n_used"] == prob.n_pts
    assert same_bits(mr.unflat(e, "align_cams"), mr.unflat(got[0], "align_cams")) and same_bits(e["centres"], got[0]["centres"])

    def writes(s):
        s.triangulate_tracks(write_points=1, want=False)
        s.transform(*mr.SIM)
    sse, cost = whole_problem_sse(prob, writes)
    assert np.array_equal(e["sse"], got[0]["sse"])
    assert abs(e["sse"][0] - sse) <= 1e-10 * sse and abs(e["sse"][1] - cost) <= 1e-10 * cost


# ------------------------------------------------------------------------------------------------ (f) the refused writes
REFUSE_WORKER = r"""
model = os.environ["MODEL"]
prob = mr.local_problem(model)[0]
cam_ref, pt_ref = mr.references(prob)
b, e = mr.shards(prob)[rank]
s = hip_backend.Solver(0)
s.comm_init(rank, world, uid)
intr = mr.upload(s, mr.take_points(prob, b, e)[0])
before = s.get_params()
msgs = {}
for name, call in (("resect", lambda: s.resect(intr=intr, write_cams=1)),
                   ("ransac", lambda: s.resect_ransac(intr=intr, seed=mr.RANSAC_SEED, write_cams=1)),
                   ("align_pts", lambda: s.align(pt_ref=pt_ref[b:e], apply=True)),
                   ("align_both", lambda: s.align(cam_ref=cam_ref, pt_ref=pt_ref[b:e], apply=True))):
    try:
        call()
        msgs[name] = None
    except hip_backend.BAHipError as err:
        msgs[name] = str(err)
after = s.get_params()
sse = mr.residuals(s, intr, "huber")
# the same calls without the write, and the write that is the same on every rank
ok = [int((s.resect(intr=intr, write_cams=0)["status"] == 0).all()), int((s.resect_ransac(intr=intr, seed=mr.RANSAC_SEED, write_cams=0)["status"] == 0).all()),
      int(s.align(cam_ref=cam_ref, pt_ref=pt_ref[b:e], apply=False)["status"] == 0)]
still = s.get_params()
al = s.align(cam_ref=cam_ref, apply=True)
moved = s.get_params()
json.dump(dict(msgs=msgs, sse=sse, ok=ok, align_status=al["status"]), open(os.path.join(OUT, f"refuse_{rank}.json"), "w"))
np.savez(os.path.join(OUT, f"refuse_{rank}.npz"), cams0=before[0], pts0=before[1], cams1=after[0], pts1=after[1], cams2=still[0], pts2=still[1],
         cams3=moved[0], pts3=moved[1])
s.close()
"""


@pytest.mark.parametrize("model", MODELS)
def test_writes_that_would_split_the_replicated_cameras_are_refused(model, tmp_path):
    """world > 1: ba_resect and ba_resect_ransac with write_cams = 1 and ba_align with apply = 1 and pt_ref return
    BA_ERR_INVALID with a message that names the field and "multi-rank", and leave the handle exactly as found (get_params
    bits; the collective residuals() still agrees on both ranks and with one rank).  The same calls without the write
    succeed, and so does align(cam_ref alone, apply = 1), which moves both ranks' cameras alike.  (Unguarded, resect with
    write_cams = 1 left the two ranks' cameras up to 1.3e-2 apart and the next ba_solve's ranks parted ways: DESIGN.md.)
    A forced communicator of ONE rank is not refused: test_forced_one_rank_communicator_gives_the_plain_handles_bits."""
    mr.launch(mr.write_worker(tmp_path / "worker.py", REFUSE_WORKER), tmp_path, env=dict(MODEL=model))
    got = load(tmp_path, "refuse")
    info = [json.load(open(tmp_path / f"refuse_{r}.json")) for r in range(2)]
    prob = mr.local_problem(model)[0]
    for r, (b, e) in enumerate(mr.shards(prob)):
        for name, field in (("resect", "write_cams"), ("ransac", "write_cams"), ("align_pts", "apply"), ("align_both", "apply")):
            msg = info[r]["msgs"][name]
            assert msg is not None, (r, name)
            assert "libba_hip error -1:" in msg and field in msg and "multi-rank" in msg, msg         # BA_ERR_INVALID
        assert "ba_resect:" in info[r]["msgs"]["resect"] and "ba_resect_ransac:" in info[r]["msgs"]["ransac"] and "pt_ref" in info[r]["msgs"]["align_pts"]
        for k in ("cams", "pts"):
            assert same_bits(got[r][k + "0"], got[r][k + "1"]) and same_bits(got[r][k + "0"], got[r][k + "2"]), (r, k)
        assert same_bits(got[r]["cams0"], prob.cams[:, :6]) and same_bits(got[r]["pts0"], prob.pts[b:e])
        assert info[r]["ok"] == [1, 1, 1] and info[r]["align_status"] == 0
    sse, cost = whole_problem_sse(prob)
    assert info[0]["sse"] == info[1]["sse"]
    assert abs(info[0]["sse"][0] - sse) <= 1e-10 * sse and abs(info[0]["sse"][1] - cost) <= 1e-10 * cost
    assert same_bits(got[0]["cams3"], got[1]["cams3"]) and not same_bits(got[0]["cams3"], got[0]["cams0"])

"""ctypes binding of ``libba_hip.so`` (C ABI: ``include/ba_hip.h``).

This is the only way the package computes anything: there is no CPU fallback.  If the
shared library has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)
or no GPU is visible, the calls raise ``BAHipError``.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .problem import BAProblem

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BA_HIP_LIB") or os.path.join(_HERE, "libba_hip.so")   # BA_HIP_LIB: another build of the same ABI

LOSS = {"linear": 0, "huber": 1, "soft_l1": 2, "cauchy": 3, "arctan": 4}    # scipy least_squares' losses (enum ba_loss)
PRECOND = {"jacobi": 0, "schur_jacobi": 1}
STATUS_NAMES = {0: "max_iters", 1: "ftol", 2: "xtol", 3: "gtol"}
PROFILE_SLOTS = 16
K_RESIDUAL, K_LINEARIZE_CAM, K_LINEARIZE_PT, K_POINT_INVERT, K_SCHUR_PT, K_SCHUR_CAM = 1, 2, 3, 4, 5, 6


class BAHipError(RuntimeError):
    pass


def loss_code(loss):
    """enum ba_loss value of a loss given by scipy name (or already by value); an unknown name raises ValueError."""
    if isinstance(loss, str):
        if loss not in LOSS:
            raise ValueError(f"unknown loss {loss!r}: expected one of {', '.join(map(repr, LOSS))}")
        return LOSS[loss]
    return loss


def precond_code(precond):
    """enum ba_precond value of a preconditioner given by name (or already by value); an unknown name raises ValueError."""
    if isinstance(precond, str):
        if precond not in PRECOND:
            raise ValueError(f"unknown preconditioner {precond!r}: expected one of {', '.join(map(repr, PRECOND))}")
        return PRECOND[precond]
    return precond


def _options(struct_type, default_fn, kw, names=None):
    """A struct_type filled by the library's default_fn and overlaid with kw.  names: option -> the function that turns a
    value given by name into its code (default: loss alone); an option the struct does not have raises TypeError."""
    names = {"loss": loss_code} if names is None else names
    o = struct_type()
    _check(default_fn(C.byref(o)))
    for k, v in kw.items():
        if k in names:
            v = names[k](v)
        if not hasattr(o, k):
            raise TypeError(f"unknown option {k}")
        setattr(o, k, v)
    return o


class BAOptions(C.Structure):
    _fields_ = [("loss", C.c_int32), ("max_iters", C.c_int32), ("f_scale", C.c_double), ("ftol", C.c_double),
                ("xtol", C.c_double), ("gtol", C.c_double), ("initial_lambda", C.c_double), ("pcg_tol", C.c_double),
                ("pcg_max_iters", C.c_int32), ("pcg_min_iters", C.c_int32), ("preconditioner", C.c_int32),
                ("jacobian_precision", C.c_int32), ("reserved0", C.c_int32), ("profile", C.c_int32),
                ("verbose", C.c_int32), ("small_solver", C.c_int32), ("pcg_model_tol", C.c_double),
                ("pcg_model_min_iters", C.c_int32), ("precond_lag", C.c_int32)]


class BASummary(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("accepted", C.c_int32), ("pcg_iterations", C.c_int32),
                ("status", C.c_int32), ("initial_sse", C.c_double), ("final_sse", C.c_double),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_lambda", C.c_double),
                ("seconds_total", C.c_double), ("seconds_linearize", C.c_double), ("seconds_pcg", C.c_double),
                ("seconds_update", C.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_}
        d["status_name"] = STATUS_NAMES.get(self.status, str(self.status))
        return d


class BAIterRecord(C.Structure):
    _fields_ = [("iteration", C.c_int32), ("accepted", C.c_int32), ("pcg_iterations", C.c_int32), ("reserved", C.c_int32),
                ("cost", C.c_double), ("cost_trial", C.c_double), ("sse_trial", C.c_double), ("lambda_", C.c_double),
                ("gain_ratio", C.c_double), ("step_norm", C.c_double), ("seconds", C.c_double)]


class BAProfile(C.Structure):
    _fields_ = [("launches", C.c_int32 * PROFILE_SLOTS), ("total_ms", C.c_double * PROFILE_SLOTS),
                ("working_launches", C.c_int32 * PROFILE_SLOTS), ("working_ms", C.c_double * PROFILE_SLOTS)]


class BATrackOptions(C.Structure):
    _fields_ = [("loss", C.c_int32), ("refine_iters", C.c_int32), ("f_scale", C.c_double), ("min_angle_deg", C.c_double),
                ("max_reproj_px", C.c_double), ("min_depth", C.c_double), ("write_points", C.c_int32), ("reserved0", C.c_int32)]


class BAResectOptions(C.Structure):
    _fields_ = [("loss", C.c_int32), ("refine_iters", C.c_int32), ("f_scale", C.c_double), ("init", C.c_int32),
                ("min_inliers", C.c_int32), ("max_reproj_px", C.c_double), ("max_rms_px", C.c_double), ("min_depth", C.c_double),
                ("write_cams", C.c_int32), ("reserved0", C.c_int32)]


class BARansacOptions(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("lo_rounds", C.c_int32), ("seed", C.c_uint64), ("max_reproj_px", C.c_double),
                ("loss", C.c_int32), ("refine_iters", C.c_int32), ("f_scale", C.c_double), ("min_inliers", C.c_int32),
                ("write_cams", C.c_int32), ("max_rms_px", C.c_double), ("min_depth", C.c_double)]


class BARelposeOptions(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("lo_rounds", C.c_int32), ("seed", C.c_uint64), ("max_epi_px", C.c_double),
                ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("min_parallax_deg", C.c_double), ("max_depth", C.c_double)]


class BAHomographyOptions(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("lo_rounds", C.c_int32), ("seed", C.c_uint64), ("max_px", C.c_double),
                ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("max_depth", C.c_double), ("ambiguity_ratio", C.c_double),
                ("min_translation", C.c_double)]


class BASim3Options(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("lo_rounds", C.c_int32), ("seed", C.c_uint64), ("max_px", C.c_double),
                ("refine_iters", C.c_int32), ("min_inliers", C.c_int32), ("with_scale", C.c_int32), ("reserved0", C.c_int32)]


class BAFundamentalOptions(C.Structure):
    _fields_ = [("n_hyp", C.c_int32), ("lo_rounds", C.c_int32), ("seed", C.c_uint64), ("max_epi_px", C.c_double),
                ("refine_iters", C.c_int32), ("min_inliers", C.c_int32)]


class BAMatchOptions(C.Structure):
    _fields_ = [("ratio", C.c_double), ("max_distance", C.c_int32), ("mutual", C.c_int32)]


class BAGuidedOptions(C.Structure):
    _fields_ = [("ratio", C.c_double), ("max_distance", C.c_int32), ("mutual", C.c_int32), ("gate", C.c_int32), ("single", C.c_int32),
                ("max_epi_px", C.c_double)]


class BAOrbOptions(C.Structure):
    _fields_ = [("scale_factor", C.c_double), ("n_features", C.c_int32), ("n_levels", C.c_int32), ("edge_threshold", C.c_int32),
                ("fast_threshold", C.c_int32)]


class BAKltOptions(C.Structure):
    _fields_ = [("half_window", C.c_int32), ("max_level", C.c_int32), ("max_iters", C.c_int32), ("reserved", C.c_int32),
                ("eps", C.c_double), ("min_eig", C.c_double), ("fb_max_px", C.c_double)]


class BAVocabOptions(C.Structure):
    _fields_ = [("branching", C.c_int32), ("levels", C.c_int32), ("iters", C.c_int32), ("min_split", C.c_int32), ("seed", C.c_uint64)]


class BATrackBuildOptions(C.Structure):
    _fields_ = [("min_length", C.c_int32), ("conflict", C.c_int32), ("max_rounds", C.c_int32), ("reserved", C.c_int32)]


GATE = {"window": 1, "epipolar": 2}   # enum BA_GATE_*
TRACKBUILD_CONFLICT = {"drop": 0, "first": 1}   # enum BA_TRACKS_*
TRACKBUILD_STATUS = {"in_track": 0, "isolated": 1, "conflict": 2, "short": 3}   # enum ba_trackbuild_status
# ba_build_tracks' counts, in order
TRACKBUILD_COUNTS = ("tracks", "members", "components", "conflict_components", "conflict_nodes", "short_components", "same_image_edges",
                     "rounds")
BOW_WEIGHTING = {"tf_idf": 0, "tf": 1}   # enum BA_BOW_*
# place recognition (csrc/ba_bow.hpp): the unit of a vector entry, the unit of idf_q, the most rows of a set in bow_transform,
# the most training rows (exclusive), the database vectors per score workgroup, the largest top_k, branching and depth
BOW_ONE, BOW_IDF_ONE, BOW_MAX_SET, BOW_MAX_TRAIN_ROWS, BOW_CHUNK, BOW_MAX_TOPK, BOW_MAX_BRANCHING, BOW_MAX_LEVELS = 1 << 30, 4096, 1 << 16, 1 << 24, 4096, 64, 32, 8

# ba_match_descriptors (csrc/ba_match.hpp): queries per workgroup, train descriptors per LDS tile, the shortest train split,
# the most splits of a pair, the most descriptors of a set, the descriptor widths
MATCH_BLOCK, MATCH_TILE, MATCH_MIN_SPLIT, MATCH_MAX_SPLITS, MATCH_MAX_SET = 256, 64, 128, 64, 1 << 20
MATCH_DESC_BYTES = (8, 16, 24, 32, 40, 48, 56, 64)
# ba_match_l2 (csrc/ba_match_l2.hpp): queries per workgroup, train descriptors per LDS tile, the shortest train split, the
# descriptor widths, and per width the chunk: the train rows of a split that share one 32-bit key range (2^ml_idx_bits)
MATCH_L2_BLOCK, MATCH_L2_TILE, MATCH_L2_MIN_SPLIT = 128, 64, 256
MATCH_L2_DESC_BYTES = (32, 64, 96, 128, 160, 192, 224, 256)
MATCH_L2_CHUNK = {32: 1024, 64: 512, 96: 256, 128: 256, 160: 256, 192: 128, 224: 128, 256: 128}
# ba_triangulate_tracks (csrc/ba_tracks.hpp): the unit vectors a long track's wave stages in LDS at a time
TRACK_STAGE = 512
# ba_covariance (csrc/ba_cov.hpp): the tile edge of the blocked dense algorithms
COV_TILE = 64
# ba_pose_graph (csrc/ba_posegraph.hpp): 8-lane teams per workgroup, threads per workgroup, the most workgroups of an edge or
# node pass, the degree above which a node is a hub, the most chunks of a hub's edge list, the shortest chunk
PG_TEAMS, PG_THREADS, PG_MAX_BLOCKS, PG_HUB_MIN, PG_HUB_CHUNKS, PG_CHUNK_MIN = 32, 256, 256, 64, 64, 16
# ba_align (csrc/ba_similarity.hpp): threads per workgroup of the reduction passes, the most workgroups (= partial rows)
ALIGN_THREADS, ALIGN_MAX_BLOCKS = 256, 128


def pg_chunk_len(deg):
    """pg_chunk_len of csrc/ba_posegraph.hpp: the edges per chunk of a hub of degree deg."""
    c = (deg + PG_HUB_CHUNKS - 1) // PG_HUB_CHUNKS
    return c if c > PG_CHUNK_MIN else PG_CHUNK_MIN


# ba_orb_extract (csrc/ba_orb.hpp): the tile of the FAST and blur kernels, the most levels, and the caps of a call
ORB_TILE_W, ORB_TILE_H, ORB_MAX_LEVELS, ORB_MAX_FEATURES, ORB_MAX_IMAGES = 64, 16, 16, 65536, 1024
ORB_STAGES = ("upload", "pyramid", "fast", "select", "harris_rank", "blur", "describe", "download")   # ba_orb_stage_times
# ba_track_klt (csrc/ba_klt.hpp): the tile of the pyramid kernel, the most levels, the largest half_window, the caps of a call
KLT_TILE_W, KLT_TILE_H, KLT_MAX_LEVELS, KLT_MAX_HALF, KLT_MAX_PAIRS, KLT_MAX_POINTS = 32, 8, 9, 15, 65535, 1 << 24
KLT_STATUS = {"ok": 0, "out": 1, "flat": 2, "fb_fail": 3}   # enum ba_klt_status
KLT_STAGES = ("upload", "pyramid", "track", "download")   # ba_klt_stage_times


class BASimilarity(C.Structure):
    _fields_ = [("s", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3)]


class BAAlignOptions(C.Structure):
    _fields_ = [("loss", C.c_int32), ("iters", C.c_int32), ("f_scale", C.c_double), ("with_scale", C.c_int32), ("apply", C.c_int32)]


class BAPosegraphOptions(C.Structure):
    _fields_ = [("loss", C.c_int32), ("max_iters", C.c_int32), ("f_scale", C.c_double), ("ftol", C.c_double),
                ("xtol", C.c_double), ("gtol", C.c_double), ("initial_lambda", C.c_double), ("pcg_tol", C.c_double),
                ("pcg_max_iters", C.c_int32), ("pcg_min_iters", C.c_int32), ("with_scale", C.c_int32), ("reserved0", C.c_int32)]


class BAAlignResult(C.Structure):
    _fields_ = [("sim", BASimilarity), ("rms", C.c_double), ("max", C.c_double), ("n_used", C.c_int32), ("status", C.c_int32)]


ALIGN_STATUS = {"ok": 0, "too_few": 1, "degenerate": 2}   # enum ba_align_status
TRACK_STATUS = {"ok": 0, "few_views": 1, "degenerate": 2, "behind": 3, "low_angle": 4, "high_error": 5}   # enum ba_track_status
RESECT_STATUS = {"ok": 0, "few_points": 1, "degenerate": 2, "behind": 3, "few_inliers": 4, "high_error": 5}   # enum ba_resect_status
RESECT_INIT = {"dlt": 0, "current": 1}   # enum ba_resect_init
RELPOSE_STATUS = {"ok": 0, "few_matches": 1, "degenerate": 2, "behind": 3, "few_inliers": 4, "low_parallax": 5}   # enum ba_relpose_status
HOMOGRAPHY_STATUS = {"ok": 0, "few_matches": 1, "degenerate": 2, "few_inliers": 3, "rotation": 4, "ambiguous": 5}   # enum ba_homography_status
SIM3_STATUS = {"ok": 0, "few_matches": 1, "degenerate": 2, "few_inliers": 3}   # enum ba_sim3_status
FUNDAMENTAL_STATUS = {"ok": 0, "few_matches": 1, "degenerate": 2, "few_inliers": 3}   # enum ba_fundamental_status


def resect_init_code(init):
    """enum ba_resect_init value of a start given by name (or already by value); an unknown name raises ValueError."""
    if isinstance(init, str):
        if init not in RESECT_INIT:
            raise ValueError(f"unknown init {init!r}: one of {sorted(RESECT_INIT)}")
        return RESECT_INIT[init]
    return init


K_TRACKS = 13
K_RESECT = 14
K_RESECT_RANSAC = 15

_lib = None

# name -> (restype, argtypes); every symbol include/ba_hip.h declares
_DP = C.POINTER(C.c_double)
_IP = C.POINTER(C.c_int32)
SYMBOLS = {
    "ba_last_error": (C.c_char_p, []),
    "ba_kernel_name": (C.c_char_p, [C.c_int]),
    "ba_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "ba_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
    "ba_destroy": (C.c_int, [C.c_void_p]),
    "ba_synchronize": (C.c_int, [C.c_void_p]),
    "ba_comm_unique_id": (C.c_int, [C.c_void_p]),
    "ba_comm_init": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "ba_set_problem": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int64, _IP, _IP, _DP, _DP, C.c_int32]),
    "ba_set_held": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8)]),
    "ba_set_shared_intrinsics": (C.c_int, [C.c_void_p, _IP]),
    "ba_set_priors": (C.c_int, [C.c_void_p, C.c_int32, _DP, _DP, _DP, _DP]),
    "ba_prior_cost": (C.c_int, [C.c_void_p, _DP, _DP, _DP]),
    "ba_set_params": (C.c_int, [C.c_void_p, _DP, _DP]),
    "ba_get_params": (C.c_int, [C.c_void_p, _DP, _DP]),
    "ba_get_rotations": (C.c_int, [C.c_void_p, _DP]),
    "ba_allgather_points": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, _DP]),
    "ba_residuals": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, _DP, _DP, _DP]),
    "ba_residuals_bal": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_double, _DP, _DP, _DP]),
    "ba_linearize_bal": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_double, _DP, _DP, _DP, _DP]),
    "ba_solve_bal": (C.c_int, [C.c_void_p, _DP, C.POINTER(BAOptions), C.POINTER(BASummary)]),
    "ba_linearize": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, _DP, _DP, _DP, _DP]),
    "ba_schur_system": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32,
                                  C.c_int32, _DP, _DP, _DP, _DP]),
    "ba_covariance": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.c_double, C.c_double, _DP, _DP, _DP]),
    "ba_default_options": (C.c_int, [C.POINTER(BAOptions)]),
    "ba_solve": (C.c_int, [C.c_void_p, C.POINTER(BAOptions), C.POINTER(BASummary)]),
    "ba_get_profile": (C.c_int, [C.c_void_p, C.POINTER(BAProfile)]),
    "ba_reset_profile": (C.c_int, [C.c_void_p]),
    "ba_time_kernel": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _DP]),
    "ba_triangulate": (C.c_int, [C.c_void_p, _DP, _DP, _DP, C.c_int64, _DP, _DP, _DP, C.POINTER(C.c_uint8)]),
    "ba_default_track_options": (C.c_int, [C.POINTER(BATrackOptions)]),
    "ba_triangulate_tracks": (C.c_int, [C.c_void_p, _DP, C.POINTER(BATrackOptions), _DP, C.POINTER(C.c_uint8), _DP, _DP, _DP]),
    "ba_default_resect_options": (C.c_int, [C.POINTER(BAResectOptions)]),
    "ba_resect": (C.c_int, [C.c_void_p, _DP, C.POINTER(BAResectOptions), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _DP,
                            C.POINTER(C.c_uint8), _IP, _DP, _DP]),
    "ba_default_ransac_options": (C.c_int, [C.POINTER(BARansacOptions)]),
    "ba_resect_ransac": (C.c_int, [C.c_void_p, _DP, C.POINTER(BARansacOptions), C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), _DP,
                                   C.POINTER(C.c_uint8), _IP, _DP, _DP, C.POINTER(C.c_uint8)]),
    "ba_default_relpose_options": (C.c_int, [C.POINTER(BARelposeOptions)]),
    "ba_relative_pose": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(BARelposeOptions), _DP, _DP,
                                   C.POINTER(C.c_uint8), _IP, _DP, _DP, _IP, C.POINTER(C.c_uint8)]),
    "ba_default_homography_options": (C.c_int, [C.POINTER(BAHomographyOptions)]),
    "ba_homography": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(BAHomographyOptions), _DP,
                                C.POINTER(C.c_uint8), _IP, _DP, _IP, C.POINTER(C.c_uint8), _IP, _DP, _DP, _DP, _DP, _IP, _DP]),
    "ba_default_sim3_options": (C.c_int, [C.POINTER(BASim3Options)]),
    "ba_sim3": (C.c_int, [C.c_void_p, _DP, C.c_int32, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(BASim3Options), _DP, _DP,
                          C.POINTER(C.c_uint8), _IP, _DP, _IP, C.POINTER(C.c_uint8), _DP]),
    "ba_default_fundamental_options": (C.c_int, [C.POINTER(BAFundamentalOptions)]),
    "ba_fundamental": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _DP, _DP, C.POINTER(BAFundamentalOptions), _DP,
                                 C.POINTER(C.c_uint8), _IP, _DP, _IP, C.POINTER(C.c_uint8), _DP, _DP]),
    "ba_default_match_options": (C.c_int, [C.POINTER(BAMatchOptions)]),
    "ba_match_descriptors": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.c_int32, _IP, _IP,
                                       C.POINTER(BAMatchOptions), C.POINTER(C.c_int64), _IP, _IP, _IP, _IP, C.POINTER(C.c_uint8), _IP]),
    "ba_match_l2": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.c_int32, _IP, _IP,
                              C.POINTER(BAMatchOptions), C.POINTER(C.c_int64), _IP, _IP, _IP, _IP, C.POINTER(C.c_uint8), _IP]),
    "ba_default_guided_options": (C.c_int, [C.POINTER(BAGuidedOptions)]),
    "ba_match_guided": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.c_int32,
                                  _IP, _IP, C.POINTER(BAGuidedOptions), C.POINTER(C.c_float), _DP, C.POINTER(C.c_int64), _IP, _IP, _IP, _IP,
                                  C.POINTER(C.c_uint8), _IP, _IP]),
    "ba_default_orb_options": (C.c_int, [C.POINTER(BAOrbOptions)]),
    "ba_orb_default_pattern": (C.c_int, [C.POINTER(C.c_int8)]),
    "ba_orb_levels": (C.c_int, [C.POINTER(BAOrbOptions), C.c_int32, C.c_int32, _IP, _IP, _DP, _IP]),
    "ba_orb_extract": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.POINTER(C.c_int8),
                                 C.POINTER(BAOrbOptions), _IP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float),
                                 C.POINTER(C.c_float), _IP, _IP, _DP, C.POINTER(C.c_uint8)]),
    "ba_orb_stage_times": (C.c_int, [C.c_void_p, C.c_int32, _DP]),
    "ba_default_klt_options": (C.c_int, [C.POINTER(BAKltOptions)]),
    "ba_klt_levels": (C.c_int, [C.POINTER(BAKltOptions), C.c_int32, C.c_int32, _IP, _IP, _IP]),
    "ba_klt_stage_times": (C.c_int, [C.c_void_p, C.c_int32, _DP]),
    "ba_track_klt": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint8), C.c_int32, _IP, C.POINTER(C.c_int64),
                               C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(BAKltOptions), C.POINTER(C.c_float),
                               C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ba_get_centres": (C.c_int, [C.c_void_p, _DP]),
    "ba_transform": (C.c_int, [C.c_void_p, C.POINTER(BASimilarity)]),
    "ba_default_align_options": (C.c_int, [C.POINTER(BAAlignOptions)]),
    "ba_align": (C.c_int, [C.c_void_p, C.POINTER(BAAlignOptions), _DP, _DP, _DP, _DP, C.POINTER(BAAlignResult), _DP, _DP]),
    "ba_default_posegraph_options": (C.c_int, [C.POINTER(BAPosegraphOptions)]),
    "ba_pose_graph": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, _IP, _IP, _DP, _DP, C.POINTER(C.c_uint8),
                                C.POINTER(BAPosegraphOptions), _DP, C.POINTER(BASummary), _DP, _DP]),
    "ba_pose_graph_trace": (C.c_int, [C.c_void_p, C.POINTER(BAIterRecord), C.c_int32, C.POINTER(C.c_int32)]),
    "ba_pose_graph_system": (C.c_int, [C.c_void_p, C.c_int32, _DP, C.c_int32, _IP, _IP, _DP, _DP, C.POINTER(C.c_uint8),
                                       C.POINTER(BAPosegraphOptions), C.c_double, _DP, _DP, _DP, _DP, _DP]),
    "ba_default_vocab_options": (C.c_int, [C.POINTER(BAVocabOptions)]),
    "ba_vocab_train": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.POINTER(BAVocabOptions),
                                 _IP, _IP, _IP]),
    "ba_vocab_size": (C.c_int, [C.c_void_p, _IP, _IP, _IP, _IP, _IP]),
    "ba_vocab_get": (C.c_int, [C.c_void_p, _IP, _IP, C.POINTER(C.c_uint8), _IP, _IP]),
    "ba_vocab_set": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _IP, _IP, C.POINTER(C.c_uint8), _IP]),
    "ba_bow_transform": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint8), C.c_int32, _IP,
                                   C.POINTER(C.c_int64), _IP, _IP]),
    "ba_bow_score": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), _IP, _IP, C.c_int32, C.POINTER(C.c_int64), _IP, _IP, _IP,
                               C.c_int32, _IP, _IP, _IP]),
    "ba_default_trackbuild_options": (C.c_int, [C.POINTER(BATrackBuildOptions)]),
    "ba_build_tracks": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.c_int64, _IP, _IP, C.POINTER(C.c_uint8),
                                  C.POINTER(BATrackBuildOptions), _IP, _IP, C.POINTER(C.c_uint8), C.POINTER(C.c_int64), _IP,
                                  C.POINTER(C.c_int64)]),
    "ba_get_trace": (C.c_int, [C.c_void_p, C.POINTER(BAIterRecord), C.c_int32, C.POINTER(C.c_int32)]),
    "ba_get_stat": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]),
    "ba_debug_occupy": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_double]),
    "ba_debug_layout": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    "ba_debug_scratch_fill": (C.c_int, [C.c_void_p, C.c_int32]),
}
# enum ba_stat (include/ba_hip.h)
STATS = {"window_mw_launches": 0, "window_lm_launches": 1, "window_fallbacks": 2, "precond_builds": 3, "precond_reuses": 4, "banded": 5,
         "cap_floor_raises": 6, "ipc_exchanges": 7, "pixels_f32": 8, "held_params": 9,
         "prior_blocks": 10, "shared_groups": 11, "scratch_bytes": 12, "scratch_allocs": 13}


def held_camera_mask(cams, n_cams, nb=6):
    """Normalise a camera hold spec to ba_set_held's uint16 (Nc,) bit masks: a bool (Nc,) array (whole cameras: all nb
    block parameters -- 6 for the pinhole, 9 for the BAL camera), a bool (Nc, 6) or (Nc, 9) array (one column per block parameter: rvec, t, then f, k1, k2), or an integer
    (Nc,) array of bit masks (bits 0-8).  None -> None.  Raises ValueError on a bad shape, dtype or bit."""
    if cams is None:
        return None
    a = np.asarray(cams)
    if a.dtype == np.bool_:
        if a.shape == (n_cams,):
            return np.where(a, (1 << nb) - 1, 0).astype(np.uint16)
        if a.ndim == 2 and a.shape[0] == n_cams and a.shape[1] in (6, 9):
            return (a.astype(np.uint16) << np.arange(a.shape[1], dtype=np.uint16)).sum(axis=1).astype(np.uint16)
        raise ValueError(f"a bool camera mask must be ({n_cams},), ({n_cams}, 6) or ({n_cams}, 9), not {a.shape}")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"camera mask must be bool or integer bit masks, not {a.dtype}")
    if a.shape != (n_cams,):
        raise ValueError(f"an integer camera mask must be ({n_cams},), not {a.shape}")
    if a.size and (a.min() < 0 or a.max() > 0x1FF):
        raise ValueError("camera mask bits must lie in 0-8 (rvec 0-2, t 3-5, f 6, k1 7, k2 8)")
    return a.astype(np.uint16)


def camera_groups(spec, n_cams):
    """Normalise a shared-intrinsics spec to ba_set_shared_intrinsics' int32 (Nc,) labels (cameras with the same label
    >= 0 share one f, k1, k2; -1: the camera's own): True (one group of all cameras), a label array (Nc,), or a list of
    index lists (group i gets label i).  None / False -> None.  Raises ValueError for an index out of range, a camera in
    two lists or a wrong length (a label below -1 is the library's to refuse: it names the camera)."""
    if spec is None or spec is False:
        return None
    if spec is True:
        return np.zeros(n_cams, dtype=np.int32)
    if isinstance(spec, np.ndarray) or (len(spec) > 0 and all(np.ndim(g) == 0 for g in spec)):
        a = np.asarray(spec)
        if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"camera group labels must be integers, not {a.dtype}")
        if a.shape != (n_cams,):
            raise ValueError(f"a camera group label array must be ({n_cams},), not {a.shape}")
        if a.size and (a.min() < np.iinfo(np.int32).min or a.max() > np.iinfo(np.int32).max):
            raise ValueError("camera group labels must fit int32")
        return a.astype(np.int32)
    labels = np.full(n_cams, -1, dtype=np.int32)
    for g, members in enumerate(spec):
        m = np.asarray(members)
        if m.ndim != 1 or (m.size and not np.issubdtype(m.dtype, np.integer)):
            raise ValueError(f"camera group {g} must be a list of camera indices")
        m = m.astype(np.int64)
        if m.size and (m.min() < 0 or m.max() >= n_cams):
            raise ValueError(f"camera group {g}: index out of range [0, {n_cams})")
        if np.unique(m).size != m.size or (labels[m] >= 0).any():
            raise ValueError(f"camera group {g}: a camera is listed twice")
        labels[m] = g
    return labels


def unpack_sym(packed, nb):
    """(..., nb (nb + 1) / 2) packed upper triangles, row by row (00 01 .. 0nb-1 11 ..), -> (..., nb, nb) symmetric."""
    packed = np.asarray(packed)
    iu = np.triu_indices(nb)
    out = np.zeros(packed.shape[:-1] + (nb, nb), dtype=packed.dtype)
    out[..., iu[0], iu[1]] = packed
    out[..., iu[1], iu[0]] = packed
    return out


def pack_sym(full, nb):
    """Inverse of unpack_sym: the upper triangles of (..., nb, nb), row by row."""
    iu = np.triu_indices(nb)
    return np.asarray(full)[..., iu[0], iu[1]]


def held_point_mask(points, n_pts):
    """Normalise a point hold spec (bool (Np,) array) to ba_set_held's uint8 flags.  None -> None."""
    if points is None:
        return None
    a = np.asarray(points)
    if a.dtype != np.bool_:
        raise ValueError(f"point mask must be a bool array, not {a.dtype}")
    if a.shape != (n_pts,):
        raise ValueError(f"point mask must be ({n_pts},), not {a.shape}")
    return a.astype(np.uint8)


def load_library():
    """Load libba_hip.so and declare every prototype.  Loud failure when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BAHipError(f"{LIB_PATH} not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950). "
                         "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise BAHipError(f"libba_hip error {rc}: {load_library().ba_last_error().decode()}")


def _dp(a):
    return a.ctypes.data_as(_DP) if a is not None else None


def _pair_inputs(pts1, pts2, pair_off, K=None, width=2):
    """What the pair-shaped calls take of (pts1, pts2, pair_off, K): K (3, 3) (None: ba_fundamental has none), the pixels (n, 2)
    and the offsets (n_pairs + 1,) int64, all contiguous (pair_off None: one pair of all matches).  width = 3: ba_sim3's (n, 3)
    points."""
    Km = None if K is None else np.ascontiguousarray(K, dtype=np.float64).reshape(3, 3)
    p1 = np.ascontiguousarray(pts1, dtype=np.float64).reshape(-1, width)
    p2 = np.ascontiguousarray(pts2, dtype=np.float64).reshape(-1, width)
    if p1.shape[0] != p2.shape[0]:
        raise ValueError("pts1 and pts2 must list the same number of points")
    off = np.array([0, p1.shape[0]], dtype=np.int64) if pair_off is None else np.ascontiguousarray(pair_off, dtype=np.int64).ravel()
    if off.size < 1 or (off.size > 1 and off[-1] != p1.shape[0]):
        raise ValueError("pair_off must have n_pairs + 1 entries and end at the number of matches")
    return Km, p1, p2, off


_F8, _I4, _U1 = np.float64, np.int32, np.uint8
_PAIR_PTR = {_F8: _DP, _I4: _IP, _U1: C.POINTER(C.c_uint8)}
_INLIER = ("match_inlier", (), _U1)
_PAIR_TAIL = [("status", (), _U1), ("n_inliers", (), _I4), ("rms_px", (), _F8)]   # three outputs every pair-shaped call has in a row


def _pair_call(fn, handle, inputs, o, spec):
    """The C call `fn` of a pair-shaped call on _pair_inputs' tuple and the options o.  spec lists the call's output arguments
    in its order as (name, shape per pair, dtype), "match_inlier" where the (n,) inlier bytes go.  Returns the outputs by name in
    that order, match_inlier last and as bool."""
    Km, p1, p2, off = inputs
    P = off.size - 1
    out = {name: np.empty((P,) + shape, dtype=dt) for name, shape, dt in spec if name != "match_inlier"}
    inl = np.zeros(p1.shape[0], dtype=np.uint8)
    ptrs = [(inl if name == "match_inlier" else out[name]).ctypes.data_as(_PAIR_PTR[dt]) for name, _, dt in spec]
    head = (handle,) if Km is None else (handle, _dp(Km))
    _check(fn(*head, P, off.ctypes.data_as(C.POINTER(C.c_int64)), _dp(p1), _dp(p2), C.byref(o), *ptrs))
    out["match_inlier"] = inl.astype(bool)
    return out


def _desc_sets(sets, width=None):
    """What the matching and place recognition calls take of a list of descriptor sets: the sets as arrays, their width, set_off and the
    concatenated descriptors.  width: the width an empty list stands for, and, when given, the one every set must have."""
    arrs = [np.asarray(a) for a in sets]
    for a in arrs:
        if a.dtype != np.uint8 or a.ndim != 2:
            raise ValueError(f"every descriptor set must be a 2-D uint8 array, not {a.dtype} with shape {a.shape}")
    widths = {a.shape[1] for a in arrs}
    if len(widths) > 1:
        raise ValueError(f"descriptor sets of different widths: {sorted(widths)} bytes")
    if widths and width is not None and widths != {width}:
        raise ValueError(f"descriptor sets of {widths.pop()} bytes, the vocabulary has {width}")
    width = widths.pop() if widths else (32 if width is None else width)
    set_off = np.zeros(len(arrs) + 1, dtype=np.int64)
    set_off[1:] = np.cumsum([a.shape[0] for a in arrs])
    desc = np.ascontiguousarray(np.concatenate(arrs, axis=0)) if arrs else np.zeros((0, width), dtype=np.uint8)
    return arrs, width, set_off, desc


def _match_inputs(sets, pairs):
    """What ba_match_descriptors and ba_match_guided take of (sets, pairs): the sets as arrays, their width, set_off, the
    concatenated descriptors, pair_query, pair_train and the number of output rows."""
    arrs, width, set_off, desc = _desc_sets(sets)
    if pairs is None:
        if len(arrs) not in (0, 2):
            raise ValueError("pairs=None needs exactly two sets (query, train)")
        pairs = [(0, 1)] if arrs else []
    pr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    ok = pr.shape[0] == 0 or (pr.min() >= 0 and pr.max() < len(arrs))
    rows = int(sum(arrs[q].shape[0] for q in pr[:, 0])) if ok else 0      # (a bad index is the library's to refuse: it names the field)
    return arrs, width, set_off, desc, np.ascontiguousarray(pr[:, 0]), np.ascontiguousarray(pr[:, 1]), rows


def _match_outputs(P, rows):
    """The result dict of a matching call, the good / n_good arrays the library writes, and the calls' common tail of output
    pointers (row_off, best, second, dist1, dist2, good, n_good)."""
    out = dict(row_off=np.zeros(P + 1, dtype=np.int64), best=np.empty(rows, dtype=np.int32), second=np.empty(rows, dtype=np.int32),
               dist1=np.empty(rows, dtype=np.int32), dist2=np.empty(rows, dtype=np.int32))
    good, n_good = np.zeros(rows, dtype=np.uint8), np.zeros(P, dtype=np.int32)
    tail = [out["row_off"].ctypes.data_as(C.POINTER(C.c_int64))] + [out[k].ctypes.data_as(_IP) for k in ("best", "second", "dist1", "dist2")]
    return out, good, n_good, tail + [good.ctypes.data_as(C.POINTER(C.c_uint8)), n_good.ctypes.data_as(_IP)]


def vocab_options(**kw) -> BAVocabOptions:
    """ba_default_vocab_options overlaid with kw (any ba_vocab_options field; an unknown one raises TypeError).  No GPU."""
    return _options(BAVocabOptions, load_library().ba_default_vocab_options, kw, names={})


def _node_array(x, name):
    """Node numbers as a contiguous int32 (n,) array.  A value that does not fit int32 raises ValueError naming the edge: narrowing
    would wrap it into a valid node (2^32 + 5 -> 5) that the library's range check could not tell from a real one."""
    x = np.asarray(x).reshape(-1)
    if x.dtype == np.int32:
        return np.ascontiguousarray(x)
    if x.size and not np.issubdtype(x.dtype, np.integer):
        raise ValueError(f"{name} must hold integers, not {x.dtype}")
    wide = x.astype(np.int64) if x.dtype != np.uint64 else x
    bad = np.nonzero((wide < -(1 << 31)) | (wide > (1 << 31) - 1))[0] if x.size else ()
    if len(bad):
        raise ValueError(f"{name}[{int(bad[0])}] = {int(wide[bad[0]])} is not a node number: it does not fit int32")
    return np.ascontiguousarray(wide, dtype=np.int32)


def _bow_csr(v, what):
    """(vec_off int64, vec_word int32, vec_val int32) of a dict of bag-of-words vectors as bow_transform returns it."""
    try:
        off, word, val = (np.asarray(v[k]) for k in ("vec_off", "vec_word", "vec_val"))
    except (KeyError, TypeError, IndexError):
        raise ValueError(f"{what} must be a dict with vec_off, vec_word and vec_val") from None
    for name, a in (("vec_off", off), ("vec_word", word), ("vec_val", val)):
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"{what}: {name} must be a 1-D integer array, not {a.dtype} with shape {a.shape}")
    if len(off) < 1 or len(word) != len(val) or int(off[-1]) != len(word):
        raise ValueError(f"{what}: vec_off must end at the number of entries of vec_word and vec_val")
    return (np.ascontiguousarray(off, dtype=np.int64), np.ascontiguousarray(word, dtype=np.int32), np.ascontiguousarray(val, dtype=np.int32))


def orb_options(**kw) -> BAOrbOptions:
    """ba_default_orb_options overlaid with kw (any ba_orb_options field; an unknown one raises TypeError)."""
    return _options(BAOrbOptions, load_library().ba_default_orb_options, kw, names={})


def orb_default_pattern():
    """ba_orb_default_pattern: the (256, 4) int8 test pairs (x1, y1, x2, y2) the extractor uses when none is given.  No GPU."""
    pat = np.zeros((256, 4), dtype=np.int8)
    _check(load_library().ba_orb_default_pattern(pat.ctypes.data_as(C.POINTER(C.c_int8))))
    return pat


def orb_levels(height, width, **opts):
    """ba_orb_levels: (level_w, level_h int32, level_scale float64, level_quota int32), n_levels entries each.  No GPU."""
    o = orb_options(**opts)
    L = max(int(o.n_levels), 0)
    w, h, q = np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.int32), np.zeros(L, dtype=np.int32)
    sc = np.zeros(L, dtype=np.float64)
    if not 1 <= L <= ORB_MAX_LEVELS:            # (the library refuses it by name; the arrays above must not be overrun)
        w = h = q = sc = None
    _check(load_library().ba_orb_levels(C.byref(o), int(height), int(width), None if w is None else w.ctypes.data_as(_IP),
                                        None if h is None else h.ctypes.data_as(_IP), _dp(sc), None if q is None else q.ctypes.data_as(_IP)))
    return w, h, sc, q


def klt_options(**kw) -> BAKltOptions:
    """ba_default_klt_options overlaid with kw (any ba_klt_options field; an unknown one raises TypeError).  No GPU."""
    return _options(BAKltOptions, load_library().ba_default_klt_options, kw, names={})


def klt_levels(height, width, **opts):
    """ba_klt_levels: (level_w, level_h) int32, one entry per pyramid level of ba_track_klt, the image first.  No GPU."""
    o = klt_options(**opts)
    w, h, n = np.zeros(KLT_MAX_LEVELS, dtype=np.int32), np.zeros(KLT_MAX_LEVELS, dtype=np.int32), C.c_int32(0)
    _check(load_library().ba_klt_levels(C.byref(o), int(height), int(width), C.byref(n), w.ctypes.data_as(_IP), h.ctypes.data_as(_IP)))
    return w[:n.value].copy(), h[:n.value].copy()


def device_count():
    n = C.c_int(0)
    _check(load_library().ba_device_count(C.byref(n)))
    return n.value


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    _check(load_library().ba_comm_unique_id(buf))
    return buf.raw


class Solver:
    """One GPU, one problem.  Thin object wrapper over the handle API."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        _check(self._lib.ba_create(int(device_id), C.byref(self._h)))
        self.n_cams = self.n_pts = self.n_obs = 0

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.ba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- multi-rank ------------------------------------------------------------------
    def comm_init(self, rank, world, unique_id: bytes | None):
        buf = C.create_string_buffer(unique_id, 128) if unique_id is not None else None
        _check(self._lib.ba_comm_init(self._h, int(rank), int(world), buf))

    # -- problem / parameters --------------------------------------------------------
    def set_problem(self, prob: BAProblem, with_params=True):
        prob.validate()
        cam_idx = np.ascontiguousarray(prob.cam_idx, dtype=np.int32)
        pt_idx = np.ascontiguousarray(prob.pt_idx, dtype=np.int32)
        uv = np.ascontiguousarray(prob.uv, dtype=np.float64)
        K4 = np.ascontiguousarray(prob.K4, dtype=np.float64)
        _check(self._lib.ba_set_problem(self._h, prob.n_cams, prob.n_pts, prob.n_obs,
                                        cam_idx.ctypes.data_as(_IP), pt_idx.ctypes.data_as(_IP), _dp(uv), _dp(K4),
                                        int(prob.fixed_cam)))
        self.n_cams, self.n_pts, self.n_obs = prob.n_cams, prob.n_pts, prob.n_obs
        self._nb = 6                           # block size a whole-camera mask covers (the BAL uploads set 9)
        self._lin = None                       # (loss, f_scale) of the last linearize(): what schur_rhs / schur_apply use
        if prob.cam_held is not None or prob.pt_held is not None:
            self.set_held(prob.cam_held, prob.pt_held)
        if prob.cam_prior is not None or prob.pt_prior is not None:
            self.set_priors(prob.cam_prior, prob.pt_prior)
        if getattr(prob, "cam_group", None) is not None:
            self.set_shared_intrinsics(prob.cam_group)
        if with_params:
            self.set_params(prob.cams, prob.pts)

    def set_priors(self, cams=None, points=None):
        """ba_set_priors: Gaussian priors 0.5 (x - mean)^T info (x - mean) added to the objective.  cams: (mean (Nc, nb),
        info (Nc, nb, nb)) or a dict camera -> (mean (nb,), info (nb, nb)), nb = 6 (rvec | t) or 9 (| f k1 k2, BAL solves);
        points: (mean (Np, 3), info (Np, 3, 3)) or a dict point -> (mean, info).  A zero block is no prior.  set_priors()
        clears both.  The priors stay with the handle across set_params and solves; set_problem clears them.  Bad specs
        raise ValueError (priors.pack_priors)."""
        from .priors import camera_prior_nb, pack_priors
        nb = camera_prior_nb(cams) or 6
        if nb not in (6, 9):
            raise ValueError(f"camera priors are written in 6 (rvec | t) or 9 (rvec | t | f k1 k2) coordinates, not {nb}")
        cp = pack_priors(cams, self.n_cams, nb, "camera")
        pp = pack_priors(points, self.n_pts, 3, "point")
        _check(self._lib.ba_set_priors(self._h, nb, None if cp is None else _dp(cp[0]), None if cp is None else _dp(cp[1]),
                                       None if pp is None else _dp(pp[0]), None if pp is None else _dp(pp[1])))

    def prior_cost(self, intr=None):
        """ba_prior_cost: (camera sum, point sum) of the prior terms at the current parameters; intr (Nc, 3) for nb = 9 priors."""
        intr = self._intr(intr)
        cc, pc = C.c_double(0), C.c_double(0)
        _check(self._lib.ba_prior_cost(self._h, _dp(intr), C.byref(cc), C.byref(pc)))
        return cc.value, pc.value

    def set_held(self, cams=None, points=None):
        """ba_set_held: parameters the solves keep constant.  cams: bool (Nc,) (whole cameras), bool (Nc, 6 | 9) (per block
        parameter) or integer bit masks (Nc,); points: bool (Np,).  A whole camera of a BAL upload (set_problem_bal,
        solve_bal) includes its f, k1, k2.  set_held() clears both.  The masks stay with the
        handle across set_params and solves; set_problem clears them."""
        cm = held_camera_mask(cams, self.n_cams, getattr(self, "_nb", 6))
        pm = held_point_mask(points, self.n_pts)
        cm = None if cm is None else np.ascontiguousarray(cm)
        pm = None if pm is None else np.ascontiguousarray(pm)
        _check(self._lib.ba_set_held(self._h, None if cm is None else cm.ctypes.data_as(C.POINTER(C.c_uint16)),
                                     None if pm is None else pm.ctypes.data_as(C.POINTER(C.c_uint8))))

    def set_shared_intrinsics(self, groups=None):
        """ba_set_shared_intrinsics: cameras that share ONE f, k1, k2 in BAL solves.  groups: True (all cameras), a label
        array (Nc,) (-1: own intrinsics), a list of index lists, or None (clear) -- see camera_groups.  The groups stay with
        the handle across set_params and solves; set_problem clears them."""
        lab = camera_groups(groups, self.n_cams)
        lab = None if lab is None else np.ascontiguousarray(lab, dtype=np.int32)
        _check(self._lib.ba_set_shared_intrinsics(self._h, None if lab is None else lab.ctypes.data_as(_IP)))

    def set_params(self, cams, pts):
        cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(self.n_cams, 6)
        pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(self.n_pts, 3)
        _check(self._lib.ba_set_params(self._h, _dp(cams), _dp(pts)))

    def get_params(self):
        cams = np.empty((self.n_cams, 6))
        pts = np.empty((self.n_pts, 3))
        _check(self._lib.ba_get_params(self._h, _dp(cams), _dp(pts)))
        return cams, pts

    def allgather_points(self, p_begin, n_total):
        """Multi-rank: the points of every shard, on every rank (collective)."""
        pts = np.empty((int(n_total), 3))
        _check(self._lib.ba_allgather_points(self._h, int(p_begin), int(n_total), _dp(pts)))
        return pts

    def get_rotations(self):
        R = np.empty((self.n_cams, 3, 3))
        _check(self._lib.ba_get_rotations(self._h, _dp(R)))
        return R

    def _intr(self, intr):
        """The (Nc, 3) float64 (f, k1, k2) array a C call reads, or None (pinhole) as it is."""
        return None if intr is None else np.ascontiguousarray(intr, dtype=np.float64).reshape(self.n_cams, 3)

    # -- kernels behind the parity entry points ----------------------------------------
    def residuals(self, loss="linear", f_scale=1.0, want_vector=True):
        r = np.empty((self.n_obs, 2)) if want_vector else None
        sse, cost = C.c_double(), C.c_double()
        _check(self._lib.ba_residuals(self._h, loss_code(loss), float(f_scale), _dp(r), C.byref(sse), C.byref(cost)))
        return r, sse.value, cost.value

    def linearize(self, loss="linear", f_scale=1.0):
        Hcc = np.empty((self.n_cams, 21)); bc = np.empty((self.n_cams, 6))
        Hpp = np.empty((self.n_pts, 6)); bp = np.empty((self.n_pts, 3))
        _check(self._lib.ba_linearize(self._h, loss_code(loss), float(f_scale), _dp(Hcc), _dp(bc), _dp(Hpp), _dp(bp)))
        self._lin = (loss, float(f_scale))
        return Hcc, bc, Hpp, bp

    def schur_system(self, lam, v=None, loss="linear", f_scale=1.0, intr=None, precond=1, lam_prev=None,
                     jacobian_precision=0):
        """ba_schur_system: the reduced camera system of one LM iteration at the current parameters.  intr None: pinhole,
        else (Nc, 3) (f, k1, k2) of the BAL camera.  v: (Nc, nb) or (n, Nc, nb) vectors, or None.  precond 0 Jacobi,
        1 Schur-Jacobi, 2 Schur-Jacobi built at lam_prev and kept.  Returns dict(g (Nc, nb), minv (Nc, nh) packed upper
        triangles, sv shaped like v or None)."""
        nb = 6 if intr is None else 9
        nh = nb * (nb + 1) // 2
        intr = self._intr(intr)
        ip = _dp(intr)
        vv, shape = None, None
        if v is not None:
            shape = np.shape(v)
            vv = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, self.n_cams, nb)
        n_vec = 0 if vv is None else vv.shape[0]
        sv = np.empty_like(vv) if vv is not None else None
        g = np.empty((self.n_cams, nb)); minv = np.empty((self.n_cams, nh))
        _check(self._lib.ba_schur_system(self._h, ip, loss_code(loss), float(f_scale), float(lam), int(precond),
                                         float(lam if lam_prev is None else lam_prev), int(jacobian_precision), n_vec,
                                         None if vv is None else _dp(vv), None if sv is None else _dp(sv), _dp(g), _dp(minv)))
        return dict(g=g, minv=minv, sv=None if sv is None else sv.reshape(shape))

    def covariance(self, loss="linear", f_scale=1.0, intr=None, full=False, rcond=0.0):
        """ba_covariance: marginal covariances of the cameras and points at the current parameters, held parameters (fixed_cam,
        set_held) conditioned on.  intr None: pinhole (nb 6), else (Nc, 3) (f, k1, k2) of the BAL camera (nb 9).  Returns
        dict(cams (Nc, nb, nb), points (Np, 3, 3), full (N, N) with N = nb Nc, or None).  Held entries are 0, points seen
        from one camera only NaN (unless they carry a prior); an undetermined gauge or point raises BAHipError
        (BA_ERR_NUMERIC).  Priors (set_priors) are part of the system: Sigma = (H + L)^-1 over the free parameters."""
        nb = 6 if intr is None else 9
        nh = nb * (nb + 1) // 2
        intr = self._intr(intr)
        ip = _dp(intr)
        cam = np.empty((self.n_cams, nh))
        pts = np.empty((self.n_pts, 6))
        fm = np.empty((nb * self.n_cams, nb * self.n_cams)) if full else None
        _check(self._lib.ba_covariance(self._h, ip, loss_code(loss), float(f_scale), float(rcond), _dp(cam), _dp(pts), _dp(fm)))
        return dict(cams=unpack_sym(cam, nb), points=unpack_sym(pts, 3), full=fm)

    def _last_linearization(self):
        lin = getattr(self, "_lin", None)
        if lin is None:
            raise BAHipError("ba_linearize first: schur_rhs / schur_apply use the loss of the last linearize()")
        return lin

    def schur_rhs(self, lam):
        loss, fs = self._last_linearization()
        return self.schur_system(lam, loss=loss, f_scale=fs)["g"]

    def schur_apply(self, lam, v):
        loss, fs = self._last_linearization()
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(self.n_cams, 6)
        return self.schur_system(lam, v, loss=loss, f_scale=fs, precond=0)["sv"]

    # -- solve -------------------------------------------------------------------------
    def default_options(self) -> BAOptions:
        o = BAOptions()
        _check(self._lib.ba_default_options(C.byref(o)))
        return o

    def solve(self, **kw):
        """kw: loss ('linear'|'huber'|'soft_l1'|'cauchy'|'arctan'), preconditioner ('jacobi'|'schur_jacobi') or any
        ba_options field.  Returns the summary as a dict."""
        o = self._options(kw)
        s = BASummary()
        _check(self._lib.ba_solve(self._h, C.byref(o), C.byref(s)))
        return s.as_dict()

    def residuals_bal(self, bal, loss="linear", f_scale=1.0, want_vector=True):
        """BAL 9-parameter camera residuals (bal.BALProblem) on the GPU: uploads the problem, returns (r, sse, cost)."""
        return self._residuals_bal_resident(self._set_bal(bal), loss, f_scale, want_vector)

    def _residuals_bal_resident(self, intr, loss="linear", f_scale=1.0, want_vector=True):
        """ba_residuals_bal on the problem the handle already holds (set_problem_bal) at its current parameters: (r, sse, cost)."""
        intr = self._intr(intr)
        r = np.empty((self.n_obs, 2)) if want_vector else None
        sse, cost = C.c_double(0), C.c_double(0)
        _check(self._lib.ba_residuals_bal(self._h, _dp(intr), loss_code(loss), float(f_scale), _dp(r), C.byref(sse), C.byref(cost)))
        return r, sse.value, cost.value

    def _set_bal(self, bal, fixed_cam=-1):
        from .problem import BAProblem
        self.set_problem(BAProblem(np.ascontiguousarray(bal.cams[:, :6]), bal.pts, bal.cam_idx, bal.pt_idx, bal.uv,
                                   np.array([1.0, 1.0, 0.0, 0.0]), fixed_cam))
        self._nb = 9
        return np.ascontiguousarray(bal.cams[:, 6:9], dtype=np.float64).copy()

    def linearize_bal(self, bal, loss="linear", f_scale=1.0, fixed_cam=-1):
        """ba_linearize_bal on a bal.BALProblem: dict(Hcc (Nc,45), bc (Nc,9), Hpp (Np,6), bp (Np,3)), packed upper triangles."""
        intr = self._set_bal(bal, fixed_cam)
        out = dict(Hcc=np.empty((self.n_cams, 45)), bc=np.empty((self.n_cams, 9)), Hpp=np.empty((self.n_pts, 6)),
                   bp=np.empty((self.n_pts, 3)))
        _check(self._lib.ba_linearize_bal(self._h, _dp(intr), loss_code(loss), float(f_scale),
                                          _dp(out["Hcc"]), _dp(out["bc"]), _dp(out["Hpp"]), _dp(out["bp"])))
        return out

    def set_problem_bal(self, bal, fixed_cam=-1):
        """Upload a bal.BALProblem once (observation lists, poses, points); returns its (Nc,3) intrinsics.  Solves on the
        resident problem: ``solve_bal_resident``; parameters are restored with ``set_params(bal.cams[:, :6], bal.pts)``."""
        return self._set_bal(bal, fixed_cam)

    def solve_bal_resident(self, intr, **kw):
        """ba_solve_bal on the problem the handle already holds: intr (Nc,3) = (f, k1, k2) per camera at the start, adjusted
        in place.  Returns the summary dict."""
        intr = self._intr(intr)
        o = self._options(kw)
        s = BASummary()
        _check(self._lib.ba_solve_bal(self._h, _dp(intr), C.byref(o), C.byref(s)))
        return s.as_dict()

    def _options(self, kw):
        """ba_default_options overlaid with kw (loss / preconditioner by name or by value, any other ba_options field)."""
        o = self.default_options()
        for k, v in kw.items():
            if k == "loss":
                v = loss_code(v)
            if k == "preconditioner":
                v = precond_code(v)
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k}")
            setattr(o, k, v)
        return o

    def solve_bal(self, bal, fixed_cam=-1, hold_intrinsics=False, held_cameras=None, held_points=None, camera_priors=None,
                  point_priors=None, shared_intrinsics=None, **kw):
        """ba_solve_bal on a bal.BALProblem (9-parameter cameras, f / k1 / k2 adjusted with the pose): returns
        (summary dict, cams (Nc,9), pts (Np,3)).  hold_intrinsics: keep every camera's f, k1, k2; held_cameras /
        held_points: as set_held (added to hold_intrinsics); camera_priors / point_priors: as set_priors;
        shared_intrinsics: as set_shared_intrinsics (the members' f, k1, k2 must be equal on entry).  kw as for solve()."""
        intr = self._set_bal(bal, fixed_cam)
        if shared_intrinsics is not None:
            self.set_shared_intrinsics(shared_intrinsics)
        if camera_priors is not None or point_priors is not None:
            self.set_priors(camera_priors, point_priors)
        cm = held_camera_mask(held_cameras, self.n_cams, 9)
        if hold_intrinsics:
            cm = (np.zeros(self.n_cams, np.uint16) if cm is None else cm) | np.uint16(0x1C0)
        if cm is not None or held_points is not None:
            self.set_held(cm, held_points)
        o = self._options(kw)
        s = BASummary()
        _check(self._lib.ba_solve_bal(self._h, _dp(intr), C.byref(o), C.byref(s)))
        cams6, pts = self.get_params()
        return s.as_dict(), np.concatenate([cams6, intr], axis=1), pts

    def triangulate(self, camera_matrix, R_rel, t_rel, pts1, pts2):
        """ba_triangulate: (n,3) points in the first camera's frame and the (n,) cheirality mask."""
        K = np.ascontiguousarray(camera_matrix, dtype=np.float64).reshape(3, 3)
        R = np.ascontiguousarray(R_rel, dtype=np.float64).reshape(3, 3)
        t = np.ascontiguousarray(t_rel, dtype=np.float64).reshape(3)
        p1 = np.ascontiguousarray(pts1, dtype=np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, dtype=np.float64).reshape(-1, 2)
        n = p1.shape[0]
        xyz = np.empty((n, 3))
        valid = np.zeros(n, dtype=np.uint8)
        _check(self._lib.ba_triangulate(self._h, _dp(K), _dp(R), _dp(t), n, _dp(p1), _dp(p2), _dp(xyz),
                                        valid.ctypes.data_as(C.POINTER(C.c_uint8))))
        return xyz, valid.astype(bool)

    def track_options(self, **kw) -> BATrackOptions:
        """ba_default_track_options overlaid with kw (loss by name or by value, any other ba_track_options field)."""
        return _options(BATrackOptions, self._lib.ba_default_track_options, kw)

    def triangulate_tracks(self, intr=None, want=True, **opts):
        """ba_triangulate_tracks: every point of the resident problem triangulated from all of its observations and the
        current cameras (intr None: pinhole; else (Nc, 3) (f, k1, k2) of the BAL camera), refined, measured and classified.
        opts: loss, refine_iters, f_scale, min_angle_deg, max_reproj_px, min_depth, write_points.  Returns dict(xyz (Np, 3),
        status (Np,) uint8 (TRACK_STATUS), angle_deg, rms_px, max_px (Np,)), the caller's point order; want=False asks for no
        output arrays (timing, or write_points alone) and returns None."""
        intr = self._intr(intr)
        ip = _dp(intr)
        o = self.track_options(**opts)
        if not want:
            _check(self._lib.ba_triangulate_tracks(self._h, ip, C.byref(o), None, None, None, None, None))
            return None
        n = self.n_pts
        out = dict(xyz=np.empty((n, 3)), status=np.empty(n, dtype=np.uint8), angle_deg=np.empty(n), rms_px=np.empty(n),
                   max_px=np.empty(n))
        _check(self._lib.ba_triangulate_tracks(self._h, ip, C.byref(o), _dp(out["xyz"]), out["status"].ctypes.data_as(C.POINTER(C.c_uint8)),
                                               _dp(out["angle_deg"]), _dp(out["rms_px"]), _dp(out["max_px"])))
        return out

    def resect_options(self, **kw) -> BAResectOptions:
        """ba_default_resect_options overlaid with kw (loss and init by name or by value, any other ba_resect_options field)."""
        return _options(BAResectOptions, self._lib.ba_default_resect_options, kw, names={"loss": loss_code, "init": resect_init_code})

    @staticmethod
    def _mask(m, n):
        """A bool (n,) mask or a list of indices -> (uint8 array, its pointer); None -> (None, None)."""
        if m is None:
            return None, None
        m = np.asarray(m)
        if m.dtype != np.bool_:
            idx, m = m.astype(np.int64).reshape(-1), np.zeros(n, dtype=bool)
            m[idx] = True
        a = np.ascontiguousarray(m.reshape(n), dtype=np.uint8)
        return a, a.ctypes.data_as(C.POINTER(C.c_uint8))

    def _resect_head(self, intr, cams, known_points):
        """What resect and resect_ransac pass alike: the pointers of intr, the camera selection and the known-point mask (a
        pointer keeps its array alive), the output dict, and the pointers of its arrays in the order of the C arguments."""
        intr = self._intr(intr)
        selp, knownp = self._mask(cams, self.n_cams)[1], self._mask(known_points, self.n_pts)[1]
        n = self.n_cams
        out = dict(poses=np.empty((n, 6)), status=np.empty(n, dtype=np.uint8), n_inliers=np.empty(n, dtype=np.int32),
                   rms_px=np.empty(n), max_px=np.empty(n))
        outp = (_dp(out["poses"]), out["status"].ctypes.data_as(C.POINTER(C.c_uint8)), out["n_inliers"].ctypes.data_as(_IP),
                _dp(out["rms_px"]), _dp(out["max_px"]))
        return (_dp(intr), selp, knownp), out, outp

    def resect(self, intr=None, cams=None, known_points=None, **opts):
        """ba_resect: the pose of every selected camera of the resident problem from its observations of the known points,
        the current points taken as they are (intr None: pinhole; else (Nc, 3) (f, k1, k2) of the BAL camera).  cams: bool
        (Nc,) mask or a list of camera indices, None = every camera; known_points: bool (Np,) mask or a list of point
        indices, None = every point.  opts: loss, refine_iters, f_scale, init ("dlt" / "current"), min_inliers,
        max_reproj_px, max_rms_px, min_depth, write_cams.  Returns dict(poses (Nc, 6) rvec | t, status (Nc,) uint8
        (RESECT_STATUS), n_inliers (Nc,) int32, rms_px, max_px (Nc,)).  Multi-rank handles: the poses come from the rank's
        shard alone, and write_cams=1 raises BAHipError (BA_ERR_INVALID) when world > 1 -- it would split the replicated
        cameras; ``resect_ransac`` alike."""
        (ip, selp, knownp), out, outp = self._resect_head(intr, cams, known_points)
        o = self.resect_options(**opts)
        _check(self._lib.ba_resect(self._h, ip, C.byref(o), selp, knownp, *outp))
        return out

    def ransac_options(self, **kw) -> BARansacOptions:
        """ba_default_ransac_options overlaid with kw (loss by name or by value, any other ba_ransac_options field)."""
        return _options(BARansacOptions, self._lib.ba_default_ransac_options, kw)

    def resect_ransac(self, intr=None, cams=None, known_points=None, **opts):
        """ba_resect_ransac: the pose of every selected camera from raw matches -- n_hyp minimal P3P samples per camera scored
        on all of its observations of the known points, then lo_rounds of (consensus, refinement on it).  intr, cams and
        known_points as ``resect``.  opts: n_hyp, lo_rounds, seed, max_reproj_px, loss, refine_iters, f_scale, min_inliers,
        write_cams, max_rms_px, min_depth.  Returns ``resect``'s dict plus obs_inlier (n_obs,) bool in the order of the
        problem's observations: the final consensus set, what to keep for the next solve
        (``triangulation.filter_observations``)."""
        (ip, selp, knownp), out, outp = self._resect_head(intr, cams, known_points)
        o = self.ransac_options(**opts)
        inl = np.zeros(self.n_obs, dtype=np.uint8)
        _check(self._lib.ba_resect_ransac(self._h, ip, C.byref(o), selp, knownp, *outp, inl.ctypes.data_as(C.POINTER(C.c_uint8))))
        out["obs_inlier"] = inl.astype(bool)
        return out

    def relpose_options(self, **kw) -> BARelposeOptions:
        """ba_default_relpose_options overlaid with kw (any ba_relpose_options field; an unknown one raises TypeError)."""
        return _options(BARelposeOptions, self._lib.ba_default_relpose_options, kw, names={})

    def relative_pose(self, K, pts1, pts2, pair_off=None, **opts):
        """ba_relative_pose: R | t (x2 ~ K (R x1 + t), |t| = 1) of every pair from raw pixel matches -- n_hyp five-point samples
        per pair scored on all of its matches, then lo_rounds of (consensus, refinement).  pts1 / pts2 (n, 2) pixels; pair_off
        (n_pairs + 1,) offsets into them (None: one pair of all matches).  opts: n_hyp, lo_rounds, seed, max_epi_px,
        refine_iters, min_inliers, min_parallax_deg, max_depth.  Returns dict(R (P, 3, 3), t (P, 3), status (P,) uint8
        (RELPOSE_STATUS), n_inliers, rms_px, parallax_deg, best_hyp (P,), match_inlier (n,) bool).  Needs no problem and
        leaves a resident one as it is."""
        return _pair_call(self._lib.ba_relative_pose, self._h, _pair_inputs(pts1, pts2, pair_off, K), self.relpose_options(**opts),
                          [("R", (3, 3), _F8), ("t", (3,), _F8)] + _PAIR_TAIL + [("parallax_deg", (), _F8), ("best_hyp", (), _I4), _INLIER])

    def homography_options(self, **kw) -> BAHomographyOptions:
        """ba_default_homography_options overlaid with kw (any ba_homography_options field; an unknown one raises TypeError)."""
        return _options(BAHomographyOptions, self._lib.ba_default_homography_options, kw, names={})

    def homography(self, K, pts1, pts2, pair_off=None, **opts):
        """ba_homography: the plane-induced H (pixels, p2 ~ H p1, unit norm, det > 0) of every pair from raw pixel matches --
        n_hyp four-point samples per pair scored on all of its matches, lo_rounds of (consensus, refinement) -- and the two
        poses it decomposes into, the better first (H~ / d2 = R + (t / d) n^T, |t| = |n| = 1).  pts1 / pts2 / pair_off as
        ``relative_pose``.  opts: n_hyp, lo_rounds, seed, max_px, refine_iters, min_inliers, max_depth, ambiguity_ratio,
        min_translation.  Returns dict(H (P, 3, 3), status (P,) uint8 (HOMOGRAPHY_STATUS), n_inliers, rms_px, best_hyp, n_pose
        (P,), match_inlier (n,) bool, R (P, 2, 3, 3), t, normal (P, 2, 3), t_over_d, votes, pose_cost (P, 2)).  Needs no problem
        and leaves a resident one as it is."""
        return _pair_call(self._lib.ba_homography, self._h, _pair_inputs(pts1, pts2, pair_off, K), self.homography_options(**opts),
                          [("H", (3, 3), _F8)] + _PAIR_TAIL + [("best_hyp", (), _I4), _INLIER, ("n_pose", (), _I4), ("R", (2, 3, 3), _F8),
                           ("t", (2, 3), _F8), ("normal", (2, 3), _F8), ("t_over_d", (2,), _F8), ("votes", (2,), _I4), ("pose_cost", (2,), _F8)])

    def sim3_options(self, **kw) -> BASim3Options:
        """ba_default_sim3_options overlaid with kw (any ba_sim3_options field; an unknown one raises TypeError)."""
        return _options(BASim3Options, self._lib.ba_default_sim3_options, kw, names={})

    def sim3(self, K, X1, X2, pair_off=None, **opts):
        """ba_sim3: the similarity X2 ~ s R X1 + t of every pair from matched 3D points in the two camera frames (z forward) --
        n_hyp three-point samples per pair scored by reprojection in both images, then lo_rounds of (consensus, closed form,
        refinement).  X1 / X2 (n, 3); pair_off as ``relative_pose``.  opts: n_hyp, lo_rounds, seed, max_px, refine_iters,
        min_inliers, with_scale.  Returns dict(sim (P, 7) rvec | t | s -- the meas of a pose-graph edge (1 -> 2) --, R (P, 3, 3), t
        (P, 3), s (P,), status (P,) uint8 (SIM3_STATUS), n_inliers, rms_px, best_hyp (P,), match_inlier (n,) bool, hessian
        (P, 7, 7): pixels^-2, in (d omega, d t, d sigma), see posegraph.edge_information).  Needs no problem and leaves a resident
        one as it is."""
        out = _pair_call(self._lib.ba_sim3, self._h, _pair_inputs(X1, X2, pair_off, K, width=3), self.sim3_options(**opts),
                         [("sim", (7,), _F8), ("R", (3, 3), _F8)] + _PAIR_TAIL + [("best_hyp", (), _I4), _INLIER, ("hessian", (7, 7), _F8)])
        inl = out.pop("match_inlier")
        out["t"], out["s"], out["match_inlier"] = out["sim"][:, 3:6].copy(), out["sim"][:, 6].copy(), inl
        return out

    def fundamental_options(self, **kw) -> BAFundamentalOptions:
        """ba_default_fundamental_options overlaid with kw (any ba_fundamental_options field; an unknown one raises TypeError)."""
        return _options(BAFundamentalOptions, self._lib.ba_default_fundamental_options, kw, names={})

    def fundamental(self, pts1, pts2, pair_off=None, **opts):
        """ba_fundamental: the fundamental matrix (pixels, p2^T F p1 = 0, unit norm, largest entry positive) of every pair from
        raw pixel matches of an uncalibrated pair -- n_hyp seven-point samples per pair scored on all of its matches, then
        lo_rounds of (consensus, refinement).  No K.  pts1 / pts2 / pair_off as ``relative_pose``.  opts: n_hyp, lo_rounds, seed,
        max_epi_px, refine_iters, min_inliers.  Returns dict(F (P, 3, 3), status (P,) uint8 (FUNDAMENTAL_STATUS), n_inliers,
        rms_px, best_hyp (P,), match_inlier (n,) bool, epipole1, epipole2 (P, 3): F e1 = 0, F^T e2 = 0, unit homogeneous pixels).
        A pair without a model has F = 0.  Needs no problem and leaves a resident one as it is."""
        return _pair_call(self._lib.ba_fundamental, self._h, _pair_inputs(pts1, pts2, pair_off), self.fundamental_options(**opts),
                          [("F", (3, 3), _F8)] + _PAIR_TAIL + [("best_hyp", (), _I4), _INLIER, ("epipole1", (3,), _F8), ("epipole2", (3,), _F8)])

    def match_options(self, **kw) -> BAMatchOptions:
        """ba_default_match_options overlaid with kw (any ba_match_options field; an unknown one raises TypeError)."""
        return _options(BAMatchOptions, self._lib.ba_default_match_options, kw, names={})

    def match_descriptors(self, sets, pairs=None, **opts):
        """ba_match_descriptors: Hamming 2-nearest-neighbours of binary descriptors with the ratio test.  sets: a list of
        (n_s, desc_bytes) uint8 arrays of one width (a multiple of 8 in 8 .. 64); pairs (P, 2) of (query set, train set), None
        with two sets: [(0, 1)].  opts: ratio, max_distance, mutual.  Returns dict(row_off (P + 1,) int64, best, second, dist1,
        dist2 (rows,) int32, good (rows,) bool, n_good (P,) int32); row row_off[p] + i is query i of pair p; -1 where there is
        no such neighbour.  ValueError for mixed widths or dtypes.  Needs no problem and leaves a resident one as it is."""
        arrs, width, set_off, desc, q, t, rows = _match_inputs(sets, pairs)
        o = self.match_options(**opts)
        out, good, n_good, tail = _match_outputs(len(q), rows)
        _check(self._lib.ba_match_descriptors(self._h, width, len(arrs), set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                              desc.ctypes.data_as(C.POINTER(C.c_uint8)), len(q), q.ctypes.data_as(_IP), t.ctypes.data_as(_IP),
                                              C.byref(o), *tail))
        out["good"] = good.astype(bool)
        out["n_good"] = n_good
        return out

    def match_l2(self, sets, pairs=None, **opts):
        """ba_match_l2: exact 2-nearest-neighbours of uint8 descriptors (SIFT as COLMAP stores it) under the squared Euclidean
        distance, with the ratio test on the squares.  sets / pairs / opts and the returned dict as match_descriptors; the
        width is a multiple of 32 in 32 .. 256, dist1 / dist2 and max_distance are SQUARED distances.  Needs no problem and
        leaves a resident one as it is."""
        arrs, width, set_off, desc, q, t, rows = _match_inputs(sets, pairs)
        o = self.match_options(**opts)
        out, good, n_good, tail = _match_outputs(len(q), rows)
        _check(self._lib.ba_match_l2(self._h, width, len(arrs), set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                     desc.ctypes.data_as(C.POINTER(C.c_uint8)), len(q), q.ctypes.data_as(_IP), t.ctypes.data_as(_IP),
                                     C.byref(o), *tail))
        out["good"] = good.astype(bool)
        out["n_good"] = n_good
        return out

    def guided_options(self, **kw) -> BAGuidedOptions:
        """ba_default_guided_options overlaid with kw (any ba_guided_options field; gate by name or value; an unknown one
        raises TypeError)."""
        return _options(BAGuidedOptions, self._lib.ba_default_guided_options, kw, names={"gate": lambda g: GATE[g] if isinstance(g, str) else g})

    def match_guided(self, sets, keypoints, pairs=None, *, window=None, fundamental=None, **opts):
        """ba_match_guided: match_descriptors over the train rows a geometric gate admits.  sets / pairs as there; keypoints: a
        list of (n_s, 2) pixel positions parallel to sets (stored as float32).  Exactly one of window ((rows, 3): predicted x,
        y in the train image and radius per query row, in row_off order; radius < 0 disables the row) and fundamental ((P, 3, 3),
        x_train^T F x_query = 0; one (3, 3) for one pair) is given and picks the gate.  opts: ratio, max_distance, mutual, single,
        max_epi_px.  Returns match_descriptors' dict plus n_cand (rows,) int32, the number of train rows the gate admits.
        ValueError for keypoints that do not fit the sets, or for both / neither of window and fundamental."""
        arrs, width, set_off, desc, q, t, rows = _match_inputs(sets, pairs)
        kps = list(keypoints)
        if len(kps) != len(arrs):
            raise ValueError(f"{len(kps)} keypoint arrays for {len(arrs)} descriptor sets")
        xy = []
        for s, (a, k) in enumerate(zip(arrs, kps)):
            k = np.asarray(k, dtype=np.float32).reshape(-1, 2) if np.size(k) else np.zeros((0, 2), dtype=np.float32)
            if k.shape[0] != a.shape[0]:
                raise ValueError(f"set {s}: {k.shape[0]} keypoints for {a.shape[0]} descriptors")
            xy.append(k)
        xy = np.ascontiguousarray(np.concatenate(xy, axis=0)) if xy else np.zeros((0, 2), dtype=np.float32)
        if (window is None) == (fundamental is None):
            raise ValueError("exactly one of window and fundamental picks the gate")
        P = len(q)
        win = F = None
        if window is not None:
            win = np.ascontiguousarray(window, dtype=np.float32).reshape(-1, 3)
            if win.shape[0] != rows:
                raise ValueError(f"window has {win.shape[0]} rows for {rows} query rows")
        else:
            F = np.ascontiguousarray(fundamental, dtype=np.float64).reshape(-1, 3, 3)
            if F.shape[0] != P:
                raise ValueError(f"{F.shape[0]} fundamental matrices for {P} pairs")
        o = self.guided_options(gate="window" if win is not None else "epipolar", **opts)
        out, good, n_good, tail = _match_outputs(P, rows)
        out["n_cand"] = np.zeros(rows, dtype=np.int32)
        fp = C.POINTER(C.c_float)
        _check(self._lib.ba_match_guided(self._h, width, len(arrs), set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                         desc.ctypes.data_as(C.POINTER(C.c_uint8)), xy.ctypes.data_as(fp), P, q.ctypes.data_as(_IP),
                                         t.ctypes.data_as(_IP), C.byref(o), None if win is None else win.ctypes.data_as(fp), _dp(F), *tail,
                                         out["n_cand"].ctypes.data_as(_IP)))
        out["good"] = good.astype(bool)
        out["n_good"] = n_good
        return out

    def extract_orb(self, images, pattern=None, **opts):
        """ba_orb_extract: ORB keypoints and descriptors of a batch of grey images -- (H, W) or (n, H, W) uint8 of one size.
        pattern: (256, 4) int8 test pairs within +-15 (None: orb_default_pattern()).  opts: scale_factor, n_features, n_levels,
        edge_threshold, fast_threshold.  Returns dict(kp_off (n + 1,) int64, n_kp (n,) int32, xy (K, 2) float32, size, angle,
        response (K,) float32, octave (K,) int32, level_xy (K, 2) int32, cs (K, 2) float64, desc (K, 32) uint8): image b owns rows
        kp_off[b] .. kp_off[b + 1] - 1.  ORB by the published algorithm, not cv2's keypoints or pattern (include/ba_hip.h).
        Needs no problem and leaves a resident one as it is."""
        imgs = np.asarray(images)
        if imgs.dtype != np.uint8 or imgs.ndim not in (2, 3):
            raise ValueError(f"images must be a uint8 array (H, W) or (n, H, W), not {imgs.dtype} with shape {imgs.shape}")
        imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
        n, H, W = imgs.shape
        pat = None
        if pattern is not None:
            pat = np.asarray(pattern)
            if pat.shape != (256, 4) or not np.issubdtype(pat.dtype, np.integer):
                raise ValueError(f"pattern must be a (256, 4) integer array, not {pat.dtype} with shape {pat.shape}")
            if pat.min() < -128 or pat.max() > 127:
                raise ValueError("pattern coordinates must fit int8")
            pat = np.ascontiguousarray(pat, dtype=np.int8)
        o = orb_options(**opts)
        N = min(max(int(o.n_features), 0), ORB_MAX_FEATURES)      # (a bad n_features is the library's to refuse: it names it)
        full = dict(xy=np.empty((n * N, 2), np.float32), size=np.empty(n * N, np.float32), angle=np.empty(n * N, np.float32),
                    response=np.empty(n * N, np.float32), octave=np.empty(n * N, np.int32), level_xy=np.empty((n * N, 2), np.int32),
                    cs=np.empty((n * N, 2), np.float64), desc=np.empty((n * N, 32), np.uint8))
        n_kp = np.zeros(n, dtype=np.int32)
        fp = C.POINTER(C.c_float)
        _check(self._lib.ba_orb_extract(self._h, n, H, W, imgs.ctypes.data_as(C.POINTER(C.c_uint8)),
                                        None if pat is None else pat.ctypes.data_as(C.POINTER(C.c_int8)), C.byref(o), n_kp.ctypes.data_as(_IP),
                                        full["xy"].ctypes.data_as(fp), full["size"].ctypes.data_as(fp), full["angle"].ctypes.data_as(fp),
                                        full["response"].ctypes.data_as(fp), full["octave"].ctypes.data_as(_IP),
                                        full["level_xy"].ctypes.data_as(_IP), _dp(full["cs"]), full["desc"].ctypes.data_as(C.POINTER(C.c_uint8))))
        keep = np.concatenate([b * N + np.arange(int(n_kp[b])) for b in range(n)]) if n else np.zeros(0, dtype=np.int64)
        out = {k: np.ascontiguousarray(v[keep]) for k, v in full.items()}
        out["n_kp"] = n_kp
        out["kp_off"] = np.concatenate([[0], np.cumsum(n_kp, dtype=np.int64)]).astype(np.int64)
        return out

    def track_klt(self, images, pairs, points, guess=None, **opts):
        """ba_track_klt: pyramidal Lucas-Kanade tracking of points from image a into image b of every pair.  images: (n, H, W)
        uint8 grey images of one size ((H, W): one image); pairs: (n_pairs, 2) image indices (a, b); points: one (n_p, 2) array
        per pair, pixels (x, y) in image a; guess: None, or the starts in image b, shaped like points.  opts: half_window,
        max_level, max_iters, eps, min_eig, fb_max_px.  Returns dict(pt_off (n_pairs + 1,) int64, next (N, 2) float32, status (N,)
        uint8 (KLT_STATUS), err, fb_err (N,) float32, levels (level_w, level_h)): pair k owns rows pt_off[k] .. pt_off[k + 1] - 1.
        Lucas-Kanade by the definition of include/ba_hip.h, not cv2's output.  Needs no problem and leaves a resident one as it is."""
        imgs = np.asarray(images)
        if imgs.dtype != np.uint8 or imgs.ndim not in (2, 3):
            raise ValueError(f"images must be a uint8 array (H, W) or (n, H, W), not {imgs.dtype} with shape {imgs.shape}")
        imgs = np.ascontiguousarray(imgs if imgs.ndim == 3 else imgs[None])
        n, H, W = imgs.shape
        pr = np.ascontiguousarray(_node_array(pairs, "pairs").reshape(-1, 2))
        pts = [np.asarray(p, dtype=np.float32).reshape(-1, 2) for p in points]
        if len(pts) != len(pr):
            raise ValueError(f"{len(pts)} point arrays for {len(pr)} pairs")
        pt_off = np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64)
        N = int(pt_off[-1])
        prev = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2)), dtype=np.float32)
        g = None
        if guess is not None:
            gs = [np.asarray(q, dtype=np.float32).reshape(-1, 2) for q in guess]
            if [len(q) for q in gs] != [len(p) for p in pts]:
                raise ValueError("guess must hold one start per point")
            g = np.ascontiguousarray(np.concatenate(gs) if gs else np.zeros((0, 2)), dtype=np.float32)
        o = klt_options(**opts)
        out = dict(pt_off=pt_off, next=np.zeros((N, 2), np.float32), status=np.zeros(N, np.uint8), err=np.full(N, np.nan, np.float32),
                   fb_err=np.full(N, np.nan, np.float32))
        fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        _check(self._lib.ba_track_klt(self._h, n, H, W, imgs.ctypes.data_as(bp), len(pr), pr.ctypes.data_as(_IP),
                                      pt_off.ctypes.data_as(C.POINTER(C.c_int64)), prev.ctypes.data_as(fp),
                                      None if g is None else g.ctypes.data_as(fp), C.byref(o), out["next"].ctypes.data_as(fp),
                                      out["status"].ctypes.data_as(bp), out["err"].ctypes.data_as(fp), out["fb_err"].ctypes.data_as(fp)))
        out["levels"] = klt_levels(H, W, **opts)
        return out

    def klt_stage_times(self, enable=None):
        """ba_klt_stage_times: enable=True / False switches the stage events of track_klt on / off (None: as it is); returns the
        stage times of the last timed call in milliseconds, a dict keyed by KLT_STAGES."""
        ms = np.zeros(len(KLT_STAGES))
        _check(self._lib.ba_klt_stage_times(self._h, -1 if enable is None else int(bool(enable)), _dp(ms)))
        return dict(zip(KLT_STAGES, ms.tolist()))

    def orb_stage_times(self, enable=None):
        """ba_orb_stage_times: enable=True / False switches the stage events of extract_orb on / off (None: as it is); returns
        the stage times of the last timed call in milliseconds, a dict keyed by ORB_STAGES."""
        ms = np.zeros(len(ORB_STAGES))
        _check(self._lib.ba_orb_stage_times(self._h, -1 if enable is None else int(bool(enable)), _dp(ms)))
        return dict(zip(ORB_STAGES, ms.tolist()))

    def train_vocabulary(self, sets, **opts):
        """ba_vocab_train: a vocabulary tree of the descriptor sets (one set per training image) by hierarchical k-majority;
        it becomes the handle's vocabulary.  opts: branching, levels, iters, min_split, seed.  Returns vocabulary()'s dict plus
        train_word (rows,) int32, the word of every training row."""
        arrs, width, set_off, desc = _desc_sets(sets)
        o = vocab_options(**opts)
        train_word = np.zeros(desc.shape[0], dtype=np.int32)
        nn, nw = C.c_int32(0), C.c_int32(0)
        _check(self._lib.ba_vocab_train(self._h, width, len(arrs), set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                        desc.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(o), train_word.ctypes.data_as(_IP),
                                        C.byref(nn), C.byref(nw)))
        out = self.vocabulary()
        out["train_word"] = train_word
        return out

    def vocabulary_size(self):
        """ba_vocab_size: dict(desc_bytes, n_nodes, n_words, branching, levels) of the resident vocabulary; zeros without one."""
        v = [C.c_int32(0) for _ in range(5)]
        _check(self._lib.ba_vocab_size(self._h, *[C.byref(x) for x in v]))
        return dict(zip(("desc_bytes", "n_nodes", "n_words", "branching", "levels"), (x.value for x in v)))

    def vocabulary(self):
        """ba_vocab_get: the resident vocabulary as a dict: desc_bytes, n_nodes, n_words, branching, levels, child0, n_child,
        word_of_node (n_nodes,) int32, node_desc (n_nodes, desc_bytes) uint8, idf_q (n_words,) int32."""
        out = self.vocabulary_size()
        nn, nw, B = out["n_nodes"], out["n_words"], out["desc_bytes"]
        out.update(child0=np.zeros(nn, dtype=np.int32), n_child=np.zeros(nn, dtype=np.int32), word_of_node=np.zeros(nn, dtype=np.int32),
                   node_desc=np.zeros((nn, B), dtype=np.uint8), idf_q=np.zeros(nw, dtype=np.int32))
        _check(self._lib.ba_vocab_get(self._h, out["child0"].ctypes.data_as(_IP), out["n_child"].ctypes.data_as(_IP),
                                      out["node_desc"].ctypes.data_as(C.POINTER(C.c_uint8)), out["word_of_node"].ctypes.data_as(_IP),
                                      out["idf_q"].ctypes.data_as(_IP)))
        return out

    def set_vocabulary(self, vocab):
        """ba_vocab_set: upload a saved or hand-made tree (child0, n_child, node_desc, idf_q of a dict or a place.Vocabulary);
        the library validates it and names the violation."""
        get = vocab.get if isinstance(vocab, dict) else lambda k: getattr(vocab, k)
        child0 = np.ascontiguousarray(get("child0"), dtype=np.int32)
        n_child = np.ascontiguousarray(get("n_child"), dtype=np.int32)
        node_desc = np.asarray(get("node_desc"))
        idf_q = np.ascontiguousarray(get("idf_q"), dtype=np.int32)
        if node_desc.dtype != np.uint8 or node_desc.ndim != 2:
            raise ValueError(f"node_desc must be a 2-D uint8 array, not {node_desc.dtype} with shape {node_desc.shape}")
        node_desc = np.ascontiguousarray(node_desc)
        if child0.ndim != 1 or child0.shape != n_child.shape or node_desc.shape[0] != child0.shape[0]:
            raise ValueError("child0, n_child and node_desc must have one entry per node")
        if idf_q.ndim != 1 or idf_q.shape[0] != int((child0 < 0).sum()):
            raise ValueError("idf_q must have one entry per leaf (child0 < 0)")
        _check(self._lib.ba_vocab_set(self._h, node_desc.shape[1], child0.shape[0], child0.ctypes.data_as(_IP), n_child.ctypes.data_as(_IP),
                                      node_desc.ctypes.data_as(C.POINTER(C.c_uint8)), idf_q.ctypes.data_as(_IP)))

    def bow_transform(self, sets, weighting="tf_idf"):
        """ba_bow_transform: the bag-of-words vector of every descriptor set under the resident vocabulary.  weighting "tf_idf"
        or "tf".  Returns dict(desc_word (rows,) int32, vec_off (n_sets + 1,) int64, vec_word, vec_val (nnz,) int32): a CSR with
        the words ascending within a set and the values summing to at most BOW_ONE."""
        if weighting not in BOW_WEIGHTING:
            raise ValueError(f"unknown weighting {weighting!r}: expected one of {', '.join(map(repr, BOW_WEIGHTING))}")
        sets = list(sets)          # (an empty list stands for no rows of the vocabulary's width; a wrong width is the library's to refuse)
        arrs, width, set_off, desc = _desc_sets(sets, None if sets else self.vocabulary_size()["desc_bytes"] or None)
        rows = desc.shape[0]
        word, vw, vv = (np.zeros(rows, dtype=np.int32) for _ in range(3))
        vec_off = np.zeros(len(arrs) + 1, dtype=np.int64)
        _check(self._lib.ba_bow_transform(self._h, width, len(arrs), set_off.ctypes.data_as(C.POINTER(C.c_int64)),
                                          desc.ctypes.data_as(C.POINTER(C.c_uint8)), BOW_WEIGHTING[weighting], word.ctypes.data_as(_IP),
                                          vec_off.ctypes.data_as(C.POINTER(C.c_int64)), vw.ctypes.data_as(_IP), vv.ctypes.data_as(_IP)))
        nnz = int(vec_off[-1])
        return dict(desc_word=word, vec_off=vec_off, vec_word=vw[:nnz].copy(), vec_val=vv[:nnz].copy())

    def bow_score(self, query, db, db_end=None, top_k=10, dense=False):
        """ba_bow_score: the L1 score sum of min(vq_i, vd_i) of every query vector against the database vectors, both dicts as
        bow_transform returns them.  db_end (nq,): query q sees the database entries j < db_end[q] only.  Returns dict(top_idx,
        top_score (nq, top_k) int32, padded with -1 / 0) and, with dense, score (nq, nd) int32."""
        q_off, q_word, q_val = _bow_csr(query, "query")
        d_off, d_word, d_val = _bow_csr(db, "db")
        nq, nd = len(q_off) - 1, len(d_off) - 1
        end = None
        if db_end is not None:
            end = np.ascontiguousarray(db_end, dtype=np.int32)
            if end.shape != (nq,):
                raise ValueError(f"db_end must have one entry per query ({nq}), not shape {end.shape}")
        top_k = int(top_k)
        if not 1 <= top_k <= BOW_MAX_TOPK:
            raise ValueError(f"top_k {top_k} is outside 1 .. {BOW_MAX_TOPK}")
        out = dict(top_idx=np.zeros((nq, top_k), dtype=np.int32), top_score=np.zeros((nq, top_k), dtype=np.int32))
        if dense:
            out["score"] = np.zeros((nq, nd), dtype=np.int32)
        p64 = C.POINTER(C.c_int64)
        _check(self._lib.ba_bow_score(self._h, nq, q_off.ctypes.data_as(p64), q_word.ctypes.data_as(_IP), q_val.ctypes.data_as(_IP), nd,
                                      d_off.ctypes.data_as(p64), d_word.ctypes.data_as(_IP), d_val.ctypes.data_as(_IP),
                                      None if end is None else end.ctypes.data_as(_IP), top_k, out["top_idx"].ctypes.data_as(_IP),
                                      out["top_score"].ctypes.data_as(_IP), out["score"].ctypes.data_as(_IP) if dense else None))
        return out

    def build_tracks(self, kp_counts, edge_a, edge_b, edge_keep=None, min_length=2, conflict="drop", max_rounds=0):
        """ba_build_tracks: feature tracks from pairwise matches.  kp_counts (n_images,): keypoints per image; node = (keypoints
        of the earlier images) + keypoint.  edge_a, edge_b (n_edges,) node pairs, one per match; edge_keep (n_edges,) or None: 0
        removes an edge (a match_inlier array as it is).  conflict "drop" (a component with two nodes in one image is no track) or
        "first" (the smallest node of every image stays).  Returns dict(kp_off (n_images + 1,) int64, node_label, node_track (N,)
        int32, node_status (N,) uint8 (TRACKBUILD_STATUS), track_off (tracks + 1,) int64, track_node (members,) int32, counts:
        dict by TRACKBUILD_COUNTS).  Everything but counts["rounds"] is a function of the set of kept edges.  Needs no problem."""
        if isinstance(conflict, str):
            if conflict not in TRACKBUILD_CONFLICT:
                raise ValueError(f"unknown conflict policy {conflict!r}: expected one of {', '.join(map(repr, TRACKBUILD_CONFLICT))}")
            conflict = TRACKBUILD_CONFLICT[conflict]
        kp_counts = np.asarray(kp_counts, dtype=np.int64).reshape(-1)
        kp_off = np.zeros(kp_counts.shape[0] + 1, dtype=np.int64)
        np.cumsum(kp_counts, out=kp_off[1:])
        a, b = _node_array(edge_a, "edge_a"), _node_array(edge_b, "edge_b")
        if a.shape != b.shape:
            raise ValueError(f"edge_a and edge_b must have the same length, not {a.shape[0]} and {b.shape[0]}")
        keep = None
        if edge_keep is not None:
            keep = np.ascontiguousarray(np.asarray(edge_keep).reshape(-1) != 0, dtype=np.uint8)
            if keep.shape != a.shape:
                raise ValueError(f"edge_keep must have one entry per edge ({a.shape[0]}), not {keep.shape[0]}")
        return self._build_tracks(kp_off, a, b, keep, BATrackBuildOptions(int(min_length), int(conflict), int(max_rounds), 0))

    def _build_tracks(self, kp_off, a, b, keep, opts):
        """The call itself on prepared arrays (kp_off int64, a / b int32, keep uint8 or None); build_tracks' dict."""
        n = max(int(kp_off[-1]), 0) if kp_off[-1] < (1 << 31) else 0      # (a refused kp_off writes nothing)
        label, track, node = (np.zeros(n, dtype=np.int32) for _ in range(3))
        status = np.zeros(n, dtype=np.uint8)
        track_off = np.zeros(n // 2 + 2, dtype=np.int64)
        counts = np.zeros(8, dtype=np.int64)
        p64, p8 = C.POINTER(C.c_int64), C.POINTER(C.c_uint8)
        _check(self._lib.ba_build_tracks(self._h, kp_off.shape[0] - 1, kp_off.ctypes.data_as(p64), a.shape[0], a.ctypes.data_as(_IP),
                                         b.ctypes.data_as(_IP), None if keep is None else keep.ctypes.data_as(p8), C.byref(opts),
                                         label.ctypes.data_as(_IP), track.ctypes.data_as(_IP), status.ctypes.data_as(p8),
                                         track_off.ctypes.data_as(p64), node.ctypes.data_as(_IP), counts.ctypes.data_as(p64)))
        n_tracks, members = int(counts[0]), int(counts[1])
        return dict(kp_off=kp_off, node_label=label, node_track=track, node_status=status, track_off=track_off[:n_tracks + 1].copy(),
                    track_node=node[:members].copy(), counts={k: int(v) for k, v in zip(TRACKBUILD_COUNTS, counts)})

    def centres(self):
        """ba_get_centres: (Nc, 3) camera centres -R_c^T t_c of the current cameras."""
        out = np.empty((self.n_cams, 3))
        _check(self._lib.ba_get_centres(self._h, _dp(out)))
        return out

    def transform(self, s=1.0, R=None, t=None):
        """ba_transform: X' = s R X + t applied to every point and camera of the current parameters (held ones included;
        residuals unchanged).  R (3, 3) defaults to the identity, t (3,) to zero.  Refused while priors are set."""
        sim = BASimilarity()
        sim.s = float(s)
        sim.R[:] = list(np.asarray(np.eye(3) if R is None else R, dtype=np.float64).reshape(9))
        sim.t[:] = list(np.asarray(np.zeros(3) if t is None else t, dtype=np.float64).reshape(3))
        _check(self._lib.ba_transform(self._h, C.byref(sim)))

    def align(self, cam_ref=None, pt_ref=None, cam_w=None, pt_w=None, loss="linear", f_scale=1.0, iters=10, with_scale=True,
              apply=False):
        """ba_align: the similarity that brings the current camera centres (cam_ref (Nc, 3)) and / or points (pt_ref (Np, 3))
        onto reference positions, weighted (cam_w, pt_w; 0 = no reference, the row may be NaN) and robust (loss / f_scale in
        the references' unit, `iters` IRLS rounds); apply=True also transforms the handle's parameters.  Returns dict(s, R
        (3, 3), t (3,), rms, max, n_used, status (ALIGN_STATUS), cam_err (Nc,) or None, pt_err (Np,) or None).  Multi-rank
        handles: apply=True with pt_ref raises BAHipError (BA_ERR_INVALID) when world > 1 (the points are the rank's own);
        cam_ref alone gives every rank the same similarity."""
        o = BAAlignOptions()
        _check(self._lib.ba_default_align_options(C.byref(o)))
        o.loss, o.iters, o.f_scale, o.with_scale, o.apply = loss_code(loss), int(iters), float(f_scale), int(bool(with_scale)), int(bool(apply))

        def arr(a, shape):
            return None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(shape)
        cam_ref, cam_w = arr(cam_ref, (self.n_cams, 3)), arr(cam_w, (self.n_cams,))
        pt_ref, pt_w = arr(pt_ref, (self.n_pts, 3)), arr(pt_w, (self.n_pts,))
        cam_err = None if cam_ref is None else np.empty(self.n_cams)
        pt_err = None if pt_ref is None else np.empty(self.n_pts)
        res = BAAlignResult()
        _check(self._lib.ba_align(self._h, C.byref(o), _dp(cam_ref), _dp(cam_w), _dp(pt_ref), _dp(pt_w), C.byref(res),
                                  _dp(cam_err), _dp(pt_err)))
        return dict(s=res.sim.s, R=np.array(res.sim.R[:]).reshape(3, 3), t=np.array(res.sim.t[:]), rms=res.rms, max=res.max,
                    n_used=res.n_used, status=res.status, cam_err=cam_err, pt_err=pt_err)

    def posegraph_options(self, **kw) -> BAPosegraphOptions:
        """ba_posegraph_options: the library's defaults overlaid with kw (loss by scipy name or code; with_scale as a bool).
        An unknown option or loss name raises ValueError."""
        o = BAPosegraphOptions()
        _check(self._lib.ba_default_posegraph_options(C.byref(o)))
        for k, v in kw.items():
            if k == "reserved0" or not hasattr(o, k):
                raise ValueError(f"unknown pose-graph option {k!r}: expected one of "
                                 f"{', '.join(n for n, _ in BAPosegraphOptions._fields_ if n != 'reserved0')}")
            setattr(o, k, loss_code(v) if k == "loss" else (int(bool(v)) if k == "with_scale" else v))
        return o

    @staticmethod
    def _posegraph_inputs(poses, edge_i, edge_j, meas, info, held):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 7)
        ei = np.ascontiguousarray(edge_i, dtype=np.int32).reshape(-1)
        ej = np.ascontiguousarray(edge_j, dtype=np.int32).reshape(-1)
        m = ei.shape[0]
        if ej.shape[0] != m:
            raise ValueError(f"edge_i has {m} entries, edge_j {ej.shape[0]}")
        meas = np.ascontiguousarray(meas, dtype=np.float64).reshape(m, 7)
        info = None if info is None else np.ascontiguousarray(info, dtype=np.float64).reshape(m, 49)
        held = None if held is None else np.ascontiguousarray(np.asarray(held) != 0, dtype=np.uint8).reshape(poses.shape[0])
        return poses, ei, ej, meas, info, held

    def pose_graph(self, poses, edge_i, edge_j, meas, info=None, held=None, **opts):
        """ba_pose_graph: Sim(3) (with_scale=False: SE(3)) pose-graph optimisation.  poses (n, 7) = rvec | t | s world-to-node,
        edges (i, j) with meas (m, 7) = S_j o S_i^-1 and info (m, 7, 7) (None: identity), held (n,) marks whole nodes kept
        constant; opts: ba_posegraph_options.  Returns the summary's fields (BASummary.as_dict) plus poses (n, 7),
        edge_chi2 (m,) and edge_weight (m,) at the returned poses.  Needs no problem and leaves a resident one as it is."""
        o = self.posegraph_options(**opts)
        poses, ei, ej, meas, info, held = self._posegraph_inputs(poses, edge_i, edge_j, meas, info, held)
        n, m = poses.shape[0], ei.shape[0]
        out, chi2, wgt = np.empty((n, 7)), np.empty(m), np.empty(m)
        sm = BASummary()
        _check(self._lib.ba_pose_graph(self._h, n, _dp(poses), m, ei.ctypes.data_as(_IP), ej.ctypes.data_as(_IP), _dp(meas), _dp(info),
                                       None if held is None else held.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(o), _dp(out),
                                       C.byref(sm), _dp(chi2), _dp(wgt)))
        d = sm.as_dict()
        d.update(poses=out, edge_chi2=chi2, edge_weight=wgt)
        return d

    def pose_graph_system(self, poses, edge_i, edge_j, meas, info=None, held=None, lam=0.0, **opts):
        """ba_pose_graph_system: at the given poses dict(e (m, 7), A, B (m, 7, 7), H (7n, 7n) = H + lam D with the held rows as
        identity rows, g (7n,)); opts gives loss, f_scale and with_scale.  7 n <= 4096."""
        o = self.posegraph_options(**opts)
        poses, ei, ej, meas, info, held = self._posegraph_inputs(poses, edge_i, edge_j, meas, info, held)
        n, m = poses.shape[0], ei.shape[0]
        dense = 7 * n if 7 * n <= 4096 else 0       # (the library refuses the call by name)
        e, A, B, H, g = np.empty((m, 7)), np.empty((m, 7, 7)), np.empty((m, 7, 7)), np.empty((dense, dense)), np.empty(7 * n)
        _check(self._lib.ba_pose_graph_system(self._h, n, _dp(poses), m, ei.ctypes.data_as(_IP), ej.ctypes.data_as(_IP), _dp(meas),
                                              _dp(info), None if held is None else held.ctypes.data_as(C.POINTER(C.c_uint8)),
                                              C.byref(o), float(lam), _dp(e), _dp(A), _dp(B), _dp(H), _dp(g)))
        return dict(e=e, A=A, B=B, H=H, g=g)

    def pose_graph_trace(self):
        """Per-iteration records of the last pose_graph on this handle (ba_pose_graph_trace): list of dicts as trace()."""
        return self._trace(self._lib.ba_pose_graph_trace)

    def trace(self):
        """Per-iteration records of the last solve (ba_get_trace): list of dicts."""
        return self._trace(self._lib.ba_get_trace)

    def _trace(self, get):
        n = C.c_int32(0)
        _check(get(self._h, None, 0, C.byref(n)))
        if n.value == 0:
            return []
        buf = (BAIterRecord * n.value)()
        _check(get(self._h, buf, n.value, C.byref(n)))
        return [dict(iteration=r.iteration, accepted=bool(r.accepted), pcg_iterations=r.pcg_iterations, cost=r.cost,
                     cost_trial=r.cost_trial, sse_trial=r.sse_trial, damping=r.lambda_, gain_ratio=r.gain_ratio,
                     step_norm=r.step_norm, seconds=r.seconds) for r in buf[:n.value]]

    def profile(self, reset=False):
        p = BAProfile()
        _check(self._lib.ba_get_profile(self._h, C.byref(p)))
        out = {}
        for i in range(PROFILE_SLOTS):
            if p.launches[i]:
                w = max(p.working_launches[i], 1)
                out[self._lib.ba_kernel_name(i).decode()] = dict(
                    launches=p.launches[i], total_ms=p.total_ms[i], mean_us=1e3 * p.total_ms[i] / p.launches[i],
                    working_launches=p.working_launches[i], working_mean_us=1e3 * p.working_ms[i] / w)
        if reset:
            _check(self._lib.ba_reset_profile(self._h))
        return out

    def time_kernel(self, slot, reps=50):
        us = C.c_double()
        _check(self._lib.ba_time_kernel(self._h, int(slot), int(reps), C.byref(us)))
        return us.value

    def synchronize(self):
        _check(self._lib.ba_synchronize(self._h))

    def stats(self):
        """Event counters of the handle (ba_get_stat): dict name -> count since the handle was created."""
        out = {}
        for name, which in STATS.items():
            v = C.c_int64(0)
            _check(self._lib.ba_get_stat(self._h, which, C.byref(v)))
            out[name] = v.value
        return out

    LAYOUT = {"pt_off": 0, "p_cam": 1, "c_pt": 2, "c_orig": 3, "offk": 4, "long_pts": 5, "blk_win": 6, "slot": 7, "scalars": 8,
              "p_uv": 9, "c_uv": 10}
    LAYOUT_SCALARS = ("lanes", "nblkP", "ppb", "nblkL", "long_spb", "long_thr", "n_long", "cam_band", "banded", "cam_segl",
                      "all_lds_pinhole", "all_lds_bal", "lds_bytes_pinhole", "lds_bytes_bal", "build_path", "mw_ok")

    def debug_layout(self, name):
        """Test hook (ba_debug_layout): one array of the layout ba_set_problem built, as numpy (scalars: a dict)."""
        which = self.LAYOUT[name]
        cap = max(2 * self.n_obs, 9 * self.n_cams, self.n_pts + 1, 16384)
        buf = np.empty(cap, dtype=np.float64 if which >= 9 else np.int32)
        n = C.c_int64(0)
        _check(self._lib.ba_debug_layout(self._h, which, buf.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        out = buf[:n.value].copy()
        return dict(zip(self.LAYOUT_SCALARS, (int(v) for v in out))) if name == "scalars" else out

    def debug_scratch_fill(self, byte):
        """Test hook (ba_debug_scratch_fill): every byte of the scratch arena set to `byte`."""
        _check(self._lib.ba_debug_scratch_fill(self._h, int(byte)))

    def debug_occupy(self, n_workgroups, lds_bytes, milliseconds):
        """Test hook (ba_debug_occupy): idle workgroups on a second stream hold compute units' LDS for a bounded time."""
        _check(self._lib.ba_debug_occupy(self._h, int(n_workgroups), int(lds_bytes), float(milliseconds)))

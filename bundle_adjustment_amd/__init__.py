"""MI355X-native sparse bundle adjustment: drop-in for the solve step of
egirgin/bundle_adjustment's ``src/bundle_adjuster.py``."""
from .map_structures import Keyframe, KeyPoint, Map, MapPoint  # noqa: F401
from .problem import BAProblem  # noqa: F401
from .bundle_adjuster import BundleAdjuster  # noqa: F401
from .pose_estimator import estimate_pose, estimate_two_view, estimate_uncalibrated, focal_from_fundamental, homography, relative_pose  # noqa: F401
# `fundamental` here stays features.fundamental(K, R, t), as before; the estimator's one-pair form is pose_estimator.fundamental
from .pose_estimator import fundamental as fundamental_matrix  # noqa: F401
from .features import BruteForceMatcher, ORBExtractor, fundamental, match, match_by_fundamental, match_by_homography, match_by_projection, match_epipolar, match_l2, quantize_descriptors  # noqa: F401
from .features import calc_optical_flow_pyr_lk, refine_matches, track  # noqa: F401
from .posegraph import close_loop, loop_measurement  # noqa: F401
from .place import KeyframeDatabase, Vocabulary, bow_vector, pair_list  # noqa: F401
from .tracks import build_tracks, chain_edges, observations, to_problem  # noqa: F401

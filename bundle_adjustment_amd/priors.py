"""Gaussian priors on camera blocks and points (``ba_set_priors``, ``include/ba_hip.h``): host-side packing and validation.

A prior is a pair ``(mean, info)``: the objective gains ``0.5 (x - mean)^T info (x - mean)``, ``x`` a camera's additive
coordinates ``rvec | t`` (``| f k1 k2`` for the BAL camera) or a point.  ``info`` is an information matrix (inverse
covariance), symmetric positive SEMIdefinite; a block of zeros is "no prior" and its mean is not read.
"""
from __future__ import annotations

import numpy as np

PSD_TOL = 1e-12        # smallest eigenvalue allowed: -PSD_TOL times the largest (the library's rule)


def info_from_sigma(sigmas):
    """Information blocks ``diag(1 / sigma^2)`` of independent standard deviations: (..., n) -> (..., n, n).
    ``inf`` gives a zero row (that coordinate gets no prior); zero or negative values raise ValueError."""
    s = np.asarray(sigmas, dtype=np.float64)
    if np.any(~(s > 0)):
        raise ValueError("standard deviations must be positive (inf = no prior on that coordinate)")
    d = 1.0 / (s * s)
    out = np.zeros(s.shape + (s.shape[-1],))
    idx = np.arange(s.shape[-1])
    out[..., idx, idx] = d
    return out


def _validate(what, mean, info):
    """The library's rules on (n, nb) means and (n, nb, nb) blocks, all blocks at once; the first offending index is named.
    Returns the mask of non-zero blocks."""
    n = info.shape[0]
    flat = info.reshape(n, -1)

    def first(bad, text):
        if bad.any():
            raise ValueError(f"{what} {int(np.argmax(bad))}: {text}")

    first(~np.isfinite(flat).all(axis=1), "non-finite entry in the information block")
    nz = flat.any(axis=1)
    first(nz & ~np.isfinite(mean).all(axis=1), "non-finite mean under a non-zero information block")
    scale = np.abs(flat).max(axis=1)
    first(np.abs(info - np.swapaxes(info, 1, 2)).reshape(n, -1).max(axis=1) > 1e-12 * scale, "the information block is not symmetric")
    if nz.any():
        w = np.linalg.eigvalsh(0.5 * (info[nz] + np.swapaxes(info[nz], 1, 2)))
        bad = (w[:, 0] < -PSD_TOL * w[:, -1]) | ~(w[:, -1] > 0.0)
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f"{what} {int(np.nonzero(nz)[0][k])}: the information block is not positive semidefinite "
                             f"(eigenvalues {w[k, 0]:g} .. {w[k, -1]:g})")
    return nz


def pack_priors(spec, n, nb, what="block"):
    """Normalise a prior spec to ``ba_set_priors``' dense arrays ``(mean (n, nb), info (n, nb (nb + 1) / 2))``, the latter
    packed upper triangles row by row.  spec: ``(mean (n, nb), info (n, nb, nb))`` or a dict ``{index: (mean (nb,),
    info (nb, nb))}`` (absent indices: no prior); None -> None.  Raises ValueError, naming the first offending index, on
    a wrong shape, an index out of range, a non-finite entry, a non-finite mean under a non-zero block or a block that
    is not positive semidefinite.  A zero block with a NaN mean passes (its mean comes back as 0)."""
    if spec is None:
        return None
    mean = np.zeros((n, nb))
    info = np.zeros((n, nb, nb))
    if isinstance(spec, dict):
        for i, (m, L) in spec.items():
            if not (isinstance(i, (int, np.integer)) and 0 <= i < n):
                raise ValueError(f"{what} {i}: index out of range [0, {n})")
            m = np.asarray(m, dtype=np.float64)
            L = np.asarray(L, dtype=np.float64)
            if m.shape != (nb,) or L.shape != (nb, nb):
                raise ValueError(f"{what} {i}: mean must be ({nb},) and info ({nb}, {nb}), not {m.shape} and {L.shape}")
            mean[i], info[i] = m, L
    else:
        try:
            m, L = spec
        except (TypeError, ValueError):
            raise ValueError(f"a {what} prior is (mean, info) or a dict index -> (mean, info)") from None
        m = np.asarray(m, dtype=np.float64)
        L = np.asarray(L, dtype=np.float64)
        if m.shape != (n, nb) or L.shape != (n, nb, nb):
            raise ValueError(f"{what} priors must be mean ({n}, {nb}) and info ({n}, {nb}, {nb}), not {m.shape} and {L.shape}")
        mean[:], info[:] = m, L
    mean[~_validate(what, mean, info)] = 0.0
    iu = np.triu_indices(nb)
    return np.ascontiguousarray(mean), np.ascontiguousarray(info[:, iu[0], iu[1]])


def camera_prior_nb(spec):
    """Block size (6 or 9) a camera prior spec is written in; None when it cannot be told (None, empty dict)."""
    if spec is None:
        return None
    if isinstance(spec, dict):
        for m, _ in spec.values():
            return int(np.asarray(m).shape[-1])
        return None
    return int(np.asarray(spec[0]).shape[-1])

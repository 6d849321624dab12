"""Pruning the Gaussians no camera sees (`Converter.contrib_begin` / `.contrib_accumulate` / `.prune` / `.prune_views`, m2s_contrib_*,
m2s_prune): the cameras — rings of orbit cameras at several elevations, because one ring does not see tops and bottoms — and the
ctypes mirror of the parameters.  The pin of the fragment weight is in include/m2s.h."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

from . import score as _sc

DEFAULT_ELEVATIONS = (-35.0, 0.0, 35.0)


class PruneParamsC(C.Structure):
    """== m2s_prune_params (include/m2s.h)."""
    _fields_ = [("min_weight", C.c_float), ("min_pixels", C.c_uint32), ("reserved", C.c_uint32)]


IMPORTANCE = {"views": 0, "area": 1}     # M2S_IMPORTANCE_*
BUDGET_COUNTS = ("before", "candidates", "kept", "threshold_key", "ties_kept", "ties")     # m2s_last_budget_counts, in order


class BudgetParamsC(C.Structure):
    """== m2s_budget_params (include/m2s.h)."""
    _fields_ = [("max_records", C.c_uint64), ("min_weight", C.c_float), ("min_pixels", C.c_uint32), ("importance", C.c_uint32),
                ("reserved", C.c_uint32)]


def orbit_cameras(scene_or_bbox, K: int, W: int, H: int, elevations: Sequence[float] = DEFAULT_ELEVATIONS):
    """K cameras round the scene at each of `elevations` (degrees, strictly between -90 and 90): score.orbit_cameras ring by ring, in
    the order of `elevations`.  -> len(elevations) * K cameras."""
    if not len(elevations):
        raise ValueError("at least one elevation")
    cams = []
    for e in elevations:
        cams += _sc.orbit_cameras(scene_or_bbox, K, W, H, float(e))
    return cams

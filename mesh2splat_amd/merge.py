"""The merge pass (`Converter.merge` / `.merge_count` / `.merge_to_budget` / `.download_merge_map`, m2s_merge): the ctypes mirror of its
parameters.  The pin — runs, segments and the moment-matched parent — is in include/m2s.h.

The defaults max_group = 4 and min_axis_dot = 0.5 are guesses: nothing in the repository has tuned them (tools/merge_probe.py reports
what they cost on one scene)."""
from __future__ import annotations

import ctypes as C

DRY_RUN = 1                                                  # M2S_MERGE_DRY_RUN
UNSIGNED_AXIS = 4                                            # M2S_MERGE_UNSIGNED_AXIS (bit 1 names nothing: flags 2 and 3 stay refused)
VALID_FLAGS = (0, DRY_RUN, UNSIGNED_AXIS, DRY_RUN | UNSIGNED_AXIS)
MAX_LEVEL = 10
MODELS = ("footprint", "gaussian")                           # M2S_MERGE_MODEL_FOOTPRINT = 0, M2S_MERGE_MODEL_GAUSSIAN = 1 (m2s_set_merge_model)
COUNTS = ("before", "after", "merged", "invalid")            # m2s_merge's out_counts, in order


class MergeParamsC(C.Structure):
    """== m2s_merge_params (include/m2s.h)."""
    _fields_ = [("level", C.c_uint32), ("max_group", C.c_uint32), ("min_axis_dot", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


def to_c(level: int, max_group: int = 4, min_axis_dot: float = 0.5, dry_run: bool = False, unsigned_axis: bool = False) -> MergeParamsC:
    c = MergeParamsC()
    c.level, c.max_group, c.min_axis_dot = int(level), int(max_group), float(min_axis_dot)
    c.flags = (DRY_RUN if dry_run else 0) | (UNSIGNED_AXIS if unsigned_axis else 0)
    return c

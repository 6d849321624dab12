"""The colour refit (`Converter.refit_begin` / `.refit_accumulate` / `.refit_apply` / `.refit_views`, m2s_refit_*): the ctypes mirrors of
its two parameter structs.  The pin of the accumulators and of the update is in include/m2s.h.

The defaults of `Converter.refit_views` — min_cover 128, min_weight_sum 1.0, two iterations — are guesses: nothing in the repository
has tuned them (tools/refit_probe.py reports what they give on one scene)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

APPLY_COUNTS = ("records", "updated", "clamped", "no_weight")     # m2s_refit_apply's out_counts, in order


@dataclass
class RefitParams:
    resolution: tuple = (1280, 720)       # W, H of the two planes
    min_cover: int = 128                  # a pixel takes part when the render's alpha byte is at least this (1..255)


class RefitParamsC(C.Structure):
    """== m2s_refit_params (include/m2s.h)."""
    _fields_ = [("resolution", C.c_int32 * 2), ("min_cover", C.c_uint32), ("reserved", C.c_uint32)]


class RefitApplyParamsC(C.Structure):
    """== m2s_refit_apply_params (include/m2s.h)."""
    _fields_ = [("step", C.c_float), ("min_weight_sum", C.c_float), ("reserved", C.c_uint32 * 2)]


def to_c(p: RefitParams) -> RefitParamsC:
    c = RefitParamsC()
    c.resolution[:] = [int(p.resolution[0]), int(p.resolution[1])]
    c.min_cover = int(p.min_cover)
    c.reserved = 0
    return c

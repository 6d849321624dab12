"""numpy restatement of m2s_records_to_world_units (the pin is in include/m2s.h): scale[0..2], columns 8..10 of the 24-float record,
divided by float32(R) in float32 — numpy's float32 division is IEEE's, correctly rounded, with subnormal quotients kept —, every other
word untouched.  The device is compared for equality of the bits.  R <= 1 (0: uploaded records) changes nothing."""
import numpy as np

F = np.float32


def to_world_units(rec, R):
    """-> a copy of rec (n, 24) float32 with columns 8..10 divided by float32(R)"""
    out = np.array(np.ascontiguousarray(rec, F).reshape(-1, 24), copy=True)
    if int(R) > 1:
        with np.errstate(all="ignore"):
            out[:, 8:11] = out[:, 8:11] / F(int(R))
        assert out.dtype == F
    return out

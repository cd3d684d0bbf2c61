"""The prior sweep's perturbation rule (include/gedepth_sweep.h) restated in numpy float32, sharing no code with the library: the
reference of tests/test_sweep_cpu.py and tests/test_sweep_gpu.py.

    drop                         : pe' = 0
    c == 0 and s == 1            : pe' = pe          (the input's bits)
    not (pe > 0)  (0, < 0, NaN)  : pe' = pe
    otherwise                    : q = 1 / pe + c;  pe' = s / q if q > 0 else 0        every operation rounded to float32
"""
import numpy as np


def variant_c(pitch_deg, cam_height=1.65):
    """The rule's c of a pitch error: formed in float64, rounded to float32 once."""
    return np.float32(np.tan(np.radians(np.float64(pitch_deg))) / np.float64(cam_height))


def perturb(pe, c, s, drop):
    """``pe``: a float32 array -> the float32 array pe' of the variant (c, s, drop)."""
    pe = np.asarray(pe)
    assert pe.dtype == np.float32
    c, s = np.float32(c), np.float32(s)
    if drop:
        return np.zeros_like(pe)
    if c == np.float32(0) and s == np.float32(1):
        return pe.copy()
    out = pe.copy()
    pos = pe > np.float32(0)                                            # False for 0, negatives and NaN
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        q = (np.float32(1) / pe[pos] + c).astype(np.float32)
        good = q > np.float32(0)
        out[pos] = np.where(good, (s / np.where(good, q, np.float32(1))).astype(np.float32), np.float32(0))
    return out


def model_plane(pe, pitch_deg, cam_height=1.65):
    """The model's own expression for the plane under a slope (ground_pixel of csrc/ground.hip), in numpy float32:
    -h / ((-h / (pe + 1e-8)) - tan(slope) + 1e-8)."""
    pe = np.asarray(pe, dtype=np.float32)
    h, eps = np.float32(cam_height), np.float32(1e-8)
    t = np.float32(np.tan(np.radians(np.float64(pitch_deg))))
    return (-h / ((-h / (pe + eps)) - t + eps)).astype(np.float32)

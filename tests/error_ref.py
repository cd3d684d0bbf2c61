"""numpy restatement of include/gedepth_error.h for the error-map tests (imported like ``eval_ref``): which pixels count, their abs-rel
error, its band and colour, the dilated picture by a brute-force window maximum, and the split's planes by a float64 sum frame by frame.
It shares no code with the library; the thresholds and the colour table are typed out again here."""
import numpy as np

import eval_ref

LIMITS = (256.0, 1e-3, 80.0)                      # depth_scale, min_depth, max_depth of the KITTI configs
T = (0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0)
RGB = ((49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248),
       (254, 224, 144), (253, 174, 97), (244, 109, 67), (215, 48, 39), (165, 0, 38))
BGR = np.array([c[::-1] for c in RGB], np.uint8)


def counted(raw, geom, rect, limits=LIMITS):
    """``(gt, mask)`` of the (Hc, Wc) window of ``geom`` = (H, W, top, left, Hc, Wc): float32 metres and ge_depth_metrics' counted pixels."""
    H, W, top, left, Hc, Wc = geom
    gt = eval_ref.window(raw, top, left, Hc, Wc, limits[0])
    return gt, eval_ref.mask_of(gt, rect, limits[1], limits[2])


def error_plane(raw, pred, geom, rect, limits=LIMITS):
    """(Hc, Wc) float32: e = |gt - pred| / gt at the counted pixels (NaN kept), -1 elsewhere."""
    gt, mask = counted(raw, geom, rect, limits)
    out = np.full(gt.shape, -1.0, np.float32)
    with np.errstate(all='ignore'):
        e = np.abs(gt - np.asarray(pred, np.float32)) / gt
    out[mask] = e[mask]
    return out


def bands(n):
    """#{ j : n >= T[j] } per element, float32 comparisons; NaN counts as +inf."""
    n = np.asarray(n, np.float32).copy()
    n[np.isnan(n)] = np.inf
    out = np.zeros(n.shape, np.int64)
    for t in T:
        out += n >= np.float32(t)
    return out


def error_image(raw, pred, frame, geom, rect, tau, radius, background, limits=LIMITS):
    """``(picture (Hc, Wc, 3) uint8 BGR, err (Hc, Wc) float32)``: the brute-force (2 radius + 1)^2 window maximum of n = e / tau over the
    counted pixels, the band's colour where there is one, else the frame's pixel (0 as it is, 1 >> 1, 2 black)."""
    H, W, top, left, Hc, Wc = geom
    err = error_plane(raw, pred, geom, rect, limits)
    mask = counted(raw, geom, rect, limits)[1]
    with np.errstate(all='ignore'):
        n = (err / np.float32(tau)).astype(np.float32)
    n[np.isnan(n)] = np.inf
    n[~mask] = -1.0
    if background == 2:
        out = np.zeros((Hc, Wc, 3), np.uint8)
    else:
        out = np.asarray(frame)[top:top + Hc, left:left + Wc].copy()
        if background == 1:
            out >>= 1
    big = np.full((Hc, Wc), -1.0, np.float32)
    for r in range(Hc):
        for c in range(Wc):
            big[r, c] = n[max(r - radius, 0):r + radius + 1, max(c - radius, 0):c + radius + 1].max()
    hit = big >= 0
    out[hit] = BGR[bands(big[hit])]
    return out, err


def accumulate(frames, geoms, rect, shape, sum0=None, count0=None, limits=LIMITS):
    """``(sum float64, count uint32)`` planes of ``shape`` after the ``(raw, pred)`` of ``frames`` in order, starting from ``sum0`` / ``count0``:
    a counted pixel with a finite e adds float64(e) and 1."""
    s = np.zeros(shape, np.float64) if sum0 is None else np.array(sum0, np.float64)
    n = np.zeros(shape, np.uint32) if count0 is None else np.array(count0, np.uint32)
    for (raw, pred), geom in zip(frames, geoms):
        e = error_plane(raw, pred, geom, rect, limits)
        ok = counted(raw, geom, rect, limits)[1] & np.isfinite(e)
        s[ok] = s[ok] + e[ok].astype(np.float64)
        n[ok] += np.uint32(1)
    return s, n

"""numpy restatement of the stratified metric sums (include/gedepth_strata.h) for their tests (imported like ``eval_ref``): the stratum of a
pixel in float32, exactly the header's expressions, and the ten sums of every stratum through ``eval_ref.sums_f64``.  It shares no code with
the library."""
import numpy as np

import eval_ref as R


def stratum_of(gt, g, edges, tol):
    """Stratum index of every pixel: ``gt`` float32 metres, ``g`` the float32 ground depth at the same pixels or None (C = 1).
    bin = #{ j : gt >= edges[j] }; on_ground = g > 0 and |gt - g| <= tol * g, all in float32; stratum = bin * C + on_ground."""
    gt = np.asarray(gt, np.float32)
    bins = np.zeros(gt.shape, np.int64)
    for e in edges:
        bins += gt >= np.float32(e)
    if g is None:
        return bins
    g = np.asarray(g, np.float32)
    assert g.dtype == gt.dtype == np.float32 and g.shape == gt.shape
    with np.errstate(invalid='ignore'):
        on = (g > np.float32(0)) & (np.abs(gt - g) <= np.float32(tol) * g)          # NaN compares false
    return bins * 2 + on


def count(edges, ground):
    return (len(edges) + 1) * (2 if ground is not None else 1)


def window_strata(raw, ground, geom, rect, edges, tol, limits=(256, 1e-3, 80)):
    """(gt, counted mask, stratum) over the (Hc, Wc) window of ``geom`` = (H, W, top, left, Hc, Wc); the stratum is -1 where the pixel does
    not count."""
    H, W, top, left, Hc, Wc = geom
    gt = R.window(raw, top, left, Hc, Wc, depth_scale=limits[0])
    mask = R.mask_of(gt, rect, limits[1], limits[2])
    g = None if ground is None else np.asarray(ground, np.float32)[top:top + Hc, left:left + Wc]
    return gt, mask, np.where(mask, stratum_of(gt, g, edges, tol), -1)


def strata_sums(raw, pred, ground, geom, rect, edges, tol, limits=(256, 1e-3, 80)):
    """(S, 10) float64: ``eval_ref.sums_f64`` over the counted pixels of every stratum."""
    gt, _, stratum = window_strata(raw, ground, geom, rect, edges, tol, limits)
    return np.stack([R.sums_f64(gt[stratum == s], pred[stratum == s]) for s in range(count(edges, ground))])


def raw_of_stratum(raw, ground, geom, rect, edges, tol, s, limits=(256, 1e-3, 80)):
    """``raw`` with the ground truth of every window pixel outside stratum ``s`` set to 0."""
    H, W, top, left, Hc, Wc = geom
    _, _, stratum = window_strata(raw, ground, geom, rect, edges, tol, limits)
    out = raw.copy()
    out[top:top + Hc, left:left + Wc] = np.where(stratum == s, raw[top:top + Hc, left:left + Wc], 0)
    return out

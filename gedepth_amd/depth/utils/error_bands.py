"""The band rule of the error images (include/gedepth_error.h) in numpy: ``error_bands`` and ``ERROR_COLOURS``.  The per-frame pictures are
painted on the device (``kernels.error_image``); this form paints the one summary picture of a split (``core.ErrorMaps.save``)."""
import numpy as np

ERROR_THRESHOLDS = np.array([0.0625, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0], np.float32)
# ColorBrewer RdYlBu-10, blue for small errors, as RGB; the pictures are written BGR (``ERROR_COLOURS[..., ::-1]``)
ERROR_COLOURS = np.array([(49, 54, 149), (69, 117, 180), (116, 173, 209), (171, 217, 233), (224, 243, 248),
                          (254, 224, 144), (253, 174, 97), (244, 109, 67), (215, 48, 39), (165, 0, 38)], np.uint8)


def error_bands(n):
    """Band 0 .. 9 of each normalised error ``n`` = abs-rel / tau (float32 arithmetic): the number of thresholds 1/16, 1/8, .. 16 that ``n``
    reaches, a value on a threshold in the upper band; a NaN counts as +inf (band 9).  Returns a uint8 array of ``n``'s shape."""
    n = np.asarray(n, dtype=np.float32)
    n = np.where(np.isnan(n), np.float32(np.inf), n)
    return (n[..., None] >= ERROR_THRESHOLDS).sum(-1).astype(np.uint8)

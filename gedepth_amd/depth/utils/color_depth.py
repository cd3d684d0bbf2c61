"""Depth colorization (depth/utils/color_depth.py of the reference): ``colorize`` maps a depth array through a matplotlib colormap to
uint8 BGR, bit-identical to the reference's ``colorize`` followed by ``Colormap.__call__(x, bytes=True)`` and ``[..., :3][..., ::-1]``.
The per-pixel work is one gfx950 launch (``ge_depth_colorize``, gedepth_amd/csrc/visualize.hip).  The default ``magma_r`` table is
committed (cmap_tables.py); any other colormap is read from matplotlib, which is then needed."""
import numpy as np
import torch

from ... import kernels
from .cmap_tables import MAGMA_R_BGR

_LUTS = {}


def colormap_table(cmap='magma_r'):
    """(N + 3, 3) uint8 numpy table of ``cmap``: N colours, then under / over / bad, BGR."""
    if cmap == 'magma_r':
        return np.frombuffer(MAGMA_R_BGR, dtype=np.uint8).reshape(-1, 3).copy()
    try:
        import matplotlib
    except ImportError as e:
        raise ImportError(f"colorize(cmap={cmap!r}) needs matplotlib to build the colormap table (only the default 'magma_r' is "
                          'built in); install matplotlib or use the default colormap') from e
    cm = matplotlib.colormaps[cmap]
    rgba = np.concatenate([cm(np.arange(cm.N), bytes=True), cm(np.array([-1.0, 2.0, np.nan]), bytes=True)])
    return np.ascontiguousarray(rgba[:, 2::-1])


def _lut(cmap, device):
    key = (cmap, device)
    if key not in _LUTS:
        _LUTS[key] = torch.from_numpy(colormap_table(cmap)).to(device)
    return _LUTS[key]


def colorize(value, cmap='magma_r', vmin=None, vmax=None):
    """Colour ``value`` (a float32 numpy array or CUDA tensor of any shape: the reference's ``(1, H, W)``, ``(N, H, W)``, ``(H, W)``)
    with ``cmap`` over ``[vmin, vmax]`` (None: the data's min / max, NaN-propagating).  Returns ``value.shape + (3,)`` uint8 in BGR order:
    numpy for a numpy input, a CUDA tensor for a CUDA tensor.  Arithmetic is numpy's float32 arithmetic; other float dtypes are converted
    to float32 first."""
    if torch.is_tensor(value):
        if not value.is_cuda:
            raise RuntimeError('colorize: gedepth_amd ops run on MI355X only; got a CPU tensor (pass a numpy array or a CUDA tensor)')
        return kernels.depth_colorize(value, vmin, vmax, _lut(cmap, value.device))
    host = np.ascontiguousarray(np.asarray(value), dtype=np.float32)
    dev = torch.device('cuda', torch.cuda.current_device())
    lut = _lut(cmap, dev)                                   # table errors (unknown cmap, no matplotlib) before the upload
    return kernels.depth_colorize(torch.from_numpy(host).to(dev), vmin, vmax, lut).cpu().numpy()

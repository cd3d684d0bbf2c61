"""Host array -> device tensor through one reused pinned buffer: the frames of apis/inference.py, the ground truth of ``pre_eval_device``."""
import numpy as np
import torch

_DTYPES = {np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16, np.dtype(np.float32): torch.float32}


class PinnedUpload:
    """``self(array, device)``: ``array`` (uint8, uint16 or float32) as a new device tensor, copied without blocking on the current
    stream.  The caller may run ahead of the device; the ORDER of the five steps below is all that keeps the host from writing the next
    array into the buffer while the copy of the last one still reads it."""

    buffer = done = None                         # pinned bytes, replaced by more when an array does not fit; event after the last copy out of them

    def __call__(self, array, device):
        if array.dtype not in _DTYPES:
            raise TypeError(f'PinnedUpload takes a uint8, uint16 or float32 array, got {array.dtype}')
        n = array.nbytes
        if self.done is not None:
            self.done.synchronize()              # 1. the last copy has read the buffer (usually long ago)
        if self.buffer is None or self.buffer.numel() < n:
            self.buffer = torch.empty(n, dtype=torch.uint8, pin_memory=True)       # 2.
        host = self.buffer[:n].view(_DTYPES[array.dtype]).view(array.shape)
        host.numpy()[...] = array                # 3.
        dev = host.to(device, non_blocking=True)  # 4.
        self.done = torch.cuda.Event()
        self.done.record()                       # 5.
        return dev

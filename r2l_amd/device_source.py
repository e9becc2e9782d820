"""What the classes that hand device batches to a training loop share (RayStore and CompactRayStore of r2l_amd/raystore.py,
PixelBatcher and ImageBatcher of r2l_amd/pixel_batch.py / image_batch.py): opening the device, two alternating sets of output
buffers, the draw counter and close().
"""
import torch

from . import _lib


class DeviceSource:
    """The contract of every source: a batch is one launch on the CURRENT stream into one of two sets of buffers, taken in turn —
    what was handed out stays valid until the second-next call, and since the launch is enqueued behind whatever read that set
    two calls ago on that stream there is no host sync and no side stream."""

    def _open(self, device, nbytes, what):
        """self.device (an indexed device for "cuda", so that tensors' devices compare equal to it) and self.nbytes; on a ROCm
        device: refuses what is more than 80 % of the free memory — what: "<class>: <what is held>" for the message — and loads
        the library."""
        self.device, self.nbytes = torch.device(device), int(nbytes)
        if self.device.type == "cuda":
            if self.device.index is None:
                self.device = torch.device("cuda", torch.cuda.current_device())
            free, _total = torch.cuda.mem_get_info(self.device)
            if self.nbytes > 0.8 * free:
                raise MemoryError("%s need %.2f GB, more than 80 %% of the %.2f GB free on %s" %
                                  (what, self.nbytes / 1e9, free / 1e9, self.device))
            self._L = _lib.load()
        self.last_ids = None
        self._slot, self._size, self._k = [None, None], [None, None], 0

    def _take(self, n):
        """(tensors, their pointers) of the set whose turn it is, sized for n by the class's _new_slot(n)."""
        k = self._k
        if self._size[k] != n:
            # (new tensors: the ones handed out two calls ago stay the caller's; the allocator is stream-ordered)
            tensors = self._new_slot(n)
            self._slot[k], self._size[k] = (tensors, tuple(_lib.ptr(t) for t in tensors)), n
        self._k = k ^ 1
        return self._slot[k]

    def close(self):
        self.last_ids = None
        self._slot, self._size = [None, None], [None, None]


class DrawCounter:
    """The number of the next draw, for a source whose batches are a function of it: a resumed run seeks to its draw."""

    draw = 0

    def seek(self, draw):
        if draw < 0:
            raise ValueError("%s.seek: negative draw" % type(self).__name__)
        self.draw = int(draw)

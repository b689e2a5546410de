"""What the GPU layer test modules (tests/test_gpu_layer*.py) share: random premultiplied pixels, and a destination image on
the device between guard rows of sentinel bytes, with or without a layer beside it.  A plain helper module, imported like
fixtures.py; the twin of tests/text_gpu.py."""
import numpy as np

SENT = 0x5b
GUARD = 3                              # rows of sentinel before and after every destination


def premultiplied(rng, shape):
    """random valid premultiplied pixels (colour <= alpha) with a share of (0, 0, 0, 0) and of opaque ones"""
    a = rng.integers(0, 256, shape + (1,))
    kind = rng.integers(0, 4, shape + (1,))
    a = np.where(kind == 0, 0, np.where(kind == 1, 255, a))
    c = rng.integers(0, 256, shape + (3,)) * a // 255
    return np.concatenate([c, a], -1).astype(np.uint8)


class Guarded:
    """a device copy of `image` (rows, stride, 4) with GUARD rows of SENT before and after it, and of `layer` (rows, stride,
    4) if there is one.  dst_skip / src_skip: pixels the device arrays are moved by, to leave the 16-byte grid.  dst and src
    are the device addresses to call with."""

    def __init__(self, image, layer=None, dst_skip=0, src_skip=0):
        import torch
        self.image, self.layer, self.src_skip = image, layer, src_skip
        guard = np.full((GUARD * image.shape[1], 4), SENT, np.uint8)
        self.first = dst_skip + guard.shape[0]
        self._dst = torch.from_numpy(np.concatenate([np.full((dst_skip, 4), SENT, np.uint8), guard, image.reshape(-1, 4), guard])).to("cuda:0")
        self.dst = self._dst.data_ptr() + 4 * self.first
        if layer is not None:
            self._src = torch.from_numpy(np.concatenate([np.zeros((src_skip, 4), np.uint8), layer.reshape(-1, 4)])).to("cuda:0")
            self.src = self._src.data_ptr() + 4 * src_skip
        torch.cuda.synchronize()

    def result(self, ctx):
        """the image after, with its guard rows checked, and the layer (kept as layer_after) against its copy"""
        ctx.sync()
        got = self._dst.cpu().numpy()
        n = self.image.shape[0] * self.image.shape[1]
        assert (got[:self.first] == SENT).all() and (got[self.first + n:] == SENT).all(), "bytes written outside the destination's rows"
        if self.layer is not None:
            self.layer_after = self._src.cpu().numpy()[self.src_skip:].reshape(self.layer.shape)
            assert np.array_equal(self.layer_after, self.layer), "the layer was written"
        return got[self.first:self.first + n].reshape(self.image.shape)

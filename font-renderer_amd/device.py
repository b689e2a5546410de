"""What every device call of the package goes through: the owner of a C handle, the context (fr_ctx) and the one round
trip host -> device -> host around calls that run on the context's stream."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L


class Handle:
    """One handle of the C ABI in `_h` and the fr_*_destroy that frees it.  close() may be called any number of times;
    an object whose creation failed has no handle and closes as a no-op."""
    _h = None

    def _open(self, destroy, create, *args) -> None:
        """create(*args, &handle), checked; `destroy` frees the handle at close()"""
        h = C.c_void_p()
        L.check(create(*args, C.byref(h)))
        self._h, self._destroy = h, destroy

    def close(self) -> None:
        if self._h:
            self._destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context(Handle):
    """fr_ctx.  stream: a hipStream_t handle (int) to launch on, e.g.
    torch.cuda.current_stream().cuda_stream, or None for a private stream."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        self._lib = L.load_library()
        self._open(self._lib.fr_ctx_destroy, self._lib.fr_ctx_create, device, C.c_void_p(stream) if stream else None)
        self.device = device

    def set_option(self, key: str, value: int) -> None:
        L.check(self._lib.fr_ctx_set_option(self._h, key.encode(), value))

    def sync(self) -> None:
        L.check(self._lib.fr_ctx_sync(self._h))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


_default_ctx: Optional[Context] = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def round_trip(ctx: Context, call, *buffers, back=0):
    """The one way host data meets a call on the context's stream.  Each of `buffers` is a uint8 host array, which is
    uploaded, or a shape, for which uninitialised device bytes are allocated; call(*device addresses) then queues its
    work, and buffers[back] comes back as a host array of the buffer's shape (back a tuple of indices: a tuple of
    arrays).  The library runs on its own stream, so
    the order is fixed: torch's uploads are complete before the call is queued (a device-wide synchronise), and the
    context's stream is drained before the copy back (ctx.sync)."""
    import torch

    where = f"cuda:{ctx.device}"
    dev = [torch.from_numpy(np.ascontiguousarray(b)).to(where) if isinstance(b, np.ndarray)
           else torch.empty(tuple(b), dtype=torch.uint8, device=where) for b in buffers]
    torch.cuda.synchronize(ctx.device)
    call(*(d.data_ptr() for d in dev))
    ctx.sync()
    if isinstance(back, tuple):
        return tuple(dev[i].cpu().numpy() for i in back)
    return dev[back].cpu().numpy()

"""What Engine and BatchEngine share when a call takes or returns device memory: the check of one buffer, the ordering of the
engine's stream against torch's, and the binder of a report's outputs.  Only marshals; torch is imported where a
tensor can turn up."""
import math

import numpy as np


class DeviceBinding:
    """Mixin of a handle with `device` (the ordinal), `stream()` (the hipStream_t of its work), `_check(status)` and
    `_ext_stream` (None until _ordered wraps the stream for torch)."""

    _owner = "engine"   # the word for the handle in messages

    def _device_buffer(self, what, x, dtypes, nbytes):
        """A device pointer (int, passed as is; a bool is not one) or a contiguous torch tensor on the handle's device, of one of
        `dtypes` (a name, a tuple of names, or None: any) and at least `nbytes` bytes: (pointer, is_tensor).  ValueError
        otherwise."""
        if isinstance(x, int) and not isinstance(x, bool):
            return x, False
        import torch
        if not isinstance(x, torch.Tensor):
            raise ValueError("%s: a device pointer (int) or a torch tensor is needed, not %s" % (what, type(x).__name__))
        if x.device.type != "cuda" or (x.device.index if x.device.index is not None else torch.cuda.current_device()) != self.device:
            raise ValueError("%s: the tensor is on %s, the %s on cuda:%d" % (what, x.device, self._owner, self.device))
        if dtypes is not None:
            dtypes = (dtypes,) if isinstance(dtypes, str) else dtypes
            if x.dtype not in [getattr(torch, d) for d in dtypes]:
                raise ValueError("%s: a %s tensor is needed, not %s" % (what, " / ".join(dtypes), x.dtype))
        if not x.is_contiguous():
            raise ValueError("%s: the tensor must be contiguous" % what)
        if x.element_size() * x.numel() < nbytes:
            raise ValueError("%s: a tensor of at least %d bytes is needed, this one has %d" % (what, nbytes, x.element_size() * x.numel()))
        return x.data_ptr(), True

    def _ordered(self, tensors, call):
        """call() enqueues on the handle's stream; with tensors, that work is ordered behind torch's current stream and torch's
        current stream behind it (no explicit sync needed on either side)."""
        if not tensors:
            return self._check(call())
        import torch
        dev = torch.device("cuda", self.device)
        if self._ext_stream is None:
            self._ext_stream = torch.cuda.ExternalStream(self.stream(), device=dev)
        cur = torch.cuda.current_stream(dev)
        self._ext_stream.wait_stream(cur)
        self._check(call())
        cur.wait_stream(self._ext_stream)

    def _bind(self, call, entries):
        """The buffers of one report call.  entries: (name, given, wanted, shape, dtype) each; `given` is what the caller passed
        (a device pointer, a torch tensor, or None: make one), or a function that makes the buffer from the handle (bodies()'s
        labels).  In this order: everything the caller gave is validated; the functions are called; what is wanted and missing
        is allocated; a tensor of another shape (a flat one, say) becomes a view of `shape` over the same storage, one that has the
        shape stays the same object.  Returns (buffers, pointers, "one of them is a tensor"), None where an entry is not wanted.
        ValueError before anything is allocated or enqueued."""
        import torch
        nbytes = [math.prod(shape) * np.dtype(dtype).itemsize for _, _, _, shape, dtype in entries]
        checked = [None if given is None or callable(given) else self._device_buffer("%s: %s" % (call, name), given, dtype, nb)
                   for (name, given, _, _, dtype), nb in zip(entries, nbytes)]
        made = [given() if callable(given) else given for _, given, _, _, _ in entries]
        bufs, ptrs, tensors = [], [], False
        for (name, _, wanted, shape, dtype), x, nb, seen in zip(entries, made, nbytes, checked):
            ptr = None
            if wanted:
                if x is None:
                    x = torch.empty(shape, dtype=getattr(torch, dtype), device=torch.device("cuda", self.device))
                ptr, t = seen or self._device_buffer("%s: %s" % (call, name), x, dtype, nb)
                if t and tuple(x.shape) != tuple(shape):
                    x = x.view(-1)[:math.prod(shape)].view(shape)
                tensors |= t
            bufs.append(x if wanted else None)
            ptrs.append(ptr)
        return bufs, ptrs, tensors

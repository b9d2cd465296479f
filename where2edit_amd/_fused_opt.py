"""What Ranger and Adam share around their one-launch kernels (csrc/multi_tensor.h is the C side of the same scheme): when the kernel
applies, and the call that hands it the tensors.  The update rules, their scalars and the `torch._foreach_*` fallbacks stay with
each optimizer."""
import ctypes
from operator import itemgetter

import torch


class FusedStep:
    """Mixin for an Optimizer with `self.fused` (None = the one-launch kernel wherever it applies, False = never, True = raise where
    it does not apply), `_fused_entry` (the library's entry point) and `_fused_state` (the state tensors it takes, in order)."""

    def _fused_applies(self, params):
        """Every parameter, gradient and state tensor of the list a contiguous fp32 tensor on one GPU, and the library there."""
        if self.fused is False:
            return False
        dev = params[0].device
        ok = dev.type == "cuda"
        state_tensors = itemgetter(*self._fused_state)
        for p in params:
            for t in (p, p.grad, *state_tensors(self.state[p])):
                ok = ok and t.device == dev and t.dtype == torch.float32 and t.is_contiguous() and t.numel() < 2 ** 31
        if ok:
            try:
                from . import _lib
                _lib.load()
            except (RuntimeError, OSError):
                ok = False
        if not ok and self.fused:
            raise RuntimeError(f"{type(self).__name__}(fused=True): needs contiguous fp32 parameters, gradients and state on one GPU, "
                               "and libw2e.so")
        return ok

    def _fused_call(self, params, int64_columns, scalars):
        """`_fused_entry(n, p, grad, *state, *int64 columns, *scalars, stream)` for at most 64 tensors per call (the kernels' table).
        `int64_columns`: functions of a parameter (its numel first).  The kernel writes through raw pointers, so the parameters'
        versions are bumped here: autograd and every cache keyed on `_version` (derived.py) must see an in-place update."""
        from . import _lib
        with torch.cuda.device(params[0].device):
            for at in range(0, len(params), 64):
                chunk = params[at:at + 64]
                n = len(chunk)
                state = [self.state[p] for p in chunk]
                tensors = [chunk, [p.grad for p in chunk], *zip(*map(itemgetter(*self._fused_state), state))]
                _lib.call(self._fused_entry, n, *[(ctypes.c_void_p * n)(*[t.data_ptr() for t in ts]) for ts in tensors],
                          *[(ctypes.c_int64 * n)(*[f(p) for p in chunk]) for f in int64_columns], *scalars, _lib.stream_ptr())
                torch.autograd.graph.increment_version(chunk)

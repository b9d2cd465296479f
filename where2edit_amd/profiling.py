"""HIP-event timing of individual C-ABI calls on the stream they are launched on (torch's current
stream).  bench.py uses it to price the dominant kernel inside the timed region; off by default.
conv_selections(): which conv and FIR kernel variant every launch of a piece of work picked."""
import os
import sys
import tempfile

import torch

_active = None


class KernelTimer:
    """with KernelTimer() as t: ... ; t.summary() -> {name: (calls, total_ms, total_work)}"""

    def __init__(self):
        self.records = []  # (name, work, start_event, end_event)
        self.enabled = True  # the caller may switch spans off for some steps (a timed event record costs ~8 us of GPU time)

    def __enter__(self):
        global _active
        _active = self
        return self

    def __exit__(self, *exc):
        global _active
        _active = None

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, work, a, b in self.records:
            calls, ms, tot = out.get(name, (0, 0.0, 0.0))
            out[name] = (calls + 1, ms + a.elapsed_time(b), tot + work)
        return out


class _Span:
    __slots__ = ("name", "work", "start")

    def __init__(self, name, work):
        self.name, self.work = name, work
        self.start = torch.cuda.Event(enable_timing=True)
        self.start.record()

    def end(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        _active.records.append((self.name, self.work, self.start, e))


def span(name, work=0.0):
    """Returns an object whose .end() closes the span, or None when timing is off."""
    return _Span(name, work) if (_active is not None and _active.enabled) else None


SELECTION_PREFIXES = ("modconv mode", "modconv variant", "modconv upblur variant", "modconv rgbfold variant", "wino_fused variant", "upfirdn variant", "  ")


def conv_selections(fn):
    """Runs fn() once with the library's `tune_print` option on and returns (lines, wino): `lines` = what w2e_modconv3x3 /
    w2e_conv3x3 / w2e_wino_fused / w2e_upfirdn2d / w2e_blur_adjoint_actbwd printed to stderr, in launch order ("modconv mode ..." with
    its "  lds-dma ..." / "  bf16x3 ..." lines, "modconv variant ...", "modconv upblur variant ..." (w2e_modconv_upblur), "modconv rgbfold variant ..." (w2e_modconv_down_rgbfold), "wino_fused variant ...", "upfirdn variant ..."), `wino` = the lines of the Winograd forms chosen on the Python side
    (functional.WINO_LOG).  tools/cfg_selections.py and the coverage census in tests/test_gpu_conv_variants.py (conv and FIR variants) both use it."""
    from . import _lib
    from . import functional as K
    torch.cuda.synchronize()
    sys.stderr.flush()
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)  # the library prints with fprintf(stderr)
        try:
            _lib.set_option("tune_print", 1)
            K.WINO_LOG = []
            fn()
            torch.cuda.synchronize()
        finally:
            _lib.set_option("tune_print", 0)
            wino, K.WINO_LOG = K.WINO_LOG, None
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        lines = [ln for ln in tmp.read().decode().splitlines() if ln.startswith(SELECTION_PREFIXES)]
    return lines, wino

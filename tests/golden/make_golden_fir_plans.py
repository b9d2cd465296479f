"""The census of FIR-dispatcher decisions behind tests/golden/fir_plans.json (tests/test_fir_plan_host.py).

census() enumerates the queries -- launches x option sets for w2e_upfirdn2d, shapes x option sets for the fused activation-backward
pass -- and record() asks a built library for the decision of each one: kernel, template flags, grid, block, LDS and the kernel's
scalar arguments (the fields of w2e_upfirdn2d_plan, include/w2e.h), and the answer of w2e_blur_adjoint_actbwd_plan.  The test walks
the same list through the library under test and compares every field, so a refactor of the dispatcher is shown on a CPU to have
changed no decision.

The committed fixture was recorded from the commit BEFORE the decision became a function of its own (w2e_upfirdn2d decided and launched
in one function, and the fused-pass condition was an inline test in functional._StyledConv.backward), with a scratch copy of that
commit's upfirdn2d.hip in which
  * every `variant(...)` call of w2e_upfirdn2d -- the statement in front of each launch -- stored (kernel id, act, planar, the grid,
    block 256, the LDS bytes and the scalar arguments of the `<<<>>>` statement that follows it) in a static array and returned 0, so
    that no launch and no W2E_LAUNCH_CHECK was reached; `if (total == 0) return 0` stored zeros;
  * w2e_blur_adjoint_actbwd returned 0 in place of its zero fill, print and launch;
  * two exported functions with the signatures of w2e_upfirdn2d_plan / w2e_blur_adjoint_actbwd_plan were appended: the first called
    w2e_upfirdn2d with never-dereferenced pointer values of the wanted alignment (0x100000 + x_misalign, 0x200000 + y_misalign; pad_y0,
    flip and the epilogue pointers 0) and copied the array out; the second evaluated the inline Python condition (width >= 256, a
    multiple of 4, 4x4 taps, deterministic = 0, tune_fuse != 0) and then called w2e_blur_adjoint_actbwd the same way: 1 where both agreed.
That file and runtime.hip were compiled into a library of their own and driven on a CPU by this script.  To re-record from a library
that has the two queries:

    python tests/golden/make_golden_fir_plans.py [path/to/libw2e.so]

Host code only: no GPU."""
import ctypes
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "fir_plans.json")
FIELDS = ("kernel", "act", "planar", "grid", "block", "lds", "arg0", "arg1", "arg2")  # W2E_FIR_PLAN_FIELDS
KERNELS = ("generic", "down4", "tile", "tile4", "blur4", "stream4")                     # W2E_FIR_*
# the distinct refusals of the dispatcher (a fragment of each message)
REFUSALS = ("bad sizes", "unsupported (max 16)", "up/down must be >= 1", "phase-planar input layout is implemented for",
            "planar input with a row pitch", "tensor too large")
LAYOUT_REFUSAL = REFUSALS[3]
DEFAULT_OPTIONS = {"deterministic": "0", "tune_blur": "0", "tune_fuse": ""}
CHANNELS = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}
BATCHES = (1, 2, 4, 8)


def planar_pitch(w):
    """W2E_PLANAR_PITCH (include/w2e.h)."""
    return ((w + 1) + 15) & ~15


def Q(planes, src, out, taps, up=1, down=1, pad_x0=0, planar=0, act=0, xmis=0, ymis=0, pitch=None):
    """One w2e_upfirdn2d_plan query, in the order of its arguments; a planar source has this library's pitch unless told otherwise."""
    if pitch is None:
        pitch = planar_pitch((src[1] - 1) >> 1) if planar else 0
    return (planes, src[0], src[1], out[0], out[1], taps[0], taps[1], up, down, pad_x0, planar, pitch, act, xmis, ymis)


def matrix_query(e):
    """The query of a FIR_MATRIX entry of tests/test_gpu_fir_variants.py (xoff / yoff are floats: misalign = 4 * off)."""
    from test_gpu_fir_variants import taps_of
    return Q(e["planes"][0] * e["planes"][1], e["src"], e["out"], taps_of(e), e["up"], e["down"], e["pad"][0], e["planar"], e["act"],
             4 * e["xoff"], 4 * e["yoff"])


def golden_queries():
    """UPFIRDN_CASES of make_golden.py: the forward call and the adjoint call functional._UpFirDn2d.backward makes."""
    from make_golden import UPFIRDN_CASES
    out = []
    for _, shape, kspec, _, up, down, pad in UPFIRDN_CASES:
        kh, kw = (5, 3) if kspec == "asym5x3" else (len(kspec), len(kspec))
        planes, (h, w) = shape[0] * shape[1], shape[2:]
        oh, ow = (h * up + pad[0] + pad[1] - kh) // down + 1, (w * up + pad[0] + pad[1] - kw) // down + 1
        out += [Q(planes, (h, w), (oh, ow), (kh, kw), up, down, pad[0]), Q(planes, (oh, ow), (h, w), (kh, kw), down, up, kw - 1 - pad[0])]
    return out


def up_blur(planes, res, act):
    """The blur after an up-sampling conv, (res + 1)^2 -> res^2, pad 1, both ways a caller can hand the source over: the phase-planar
    image (which the launcher takes or refuses: w2e_upfirdn2d_planar_ok is that rule) and its re-interleaved copy."""
    return [Q(planes, (res + 1, res + 1), (res, res), (4, 4), pad_x0=1, planar=planar, act=act) for planar in (1, 0)]


def generator_queries():
    """Every FIR launch of a generator step at sizes 8 ... 1024: per up-sampling StyledConv the blur with and without its epilogue and,
    backward, the adjoint blur onto the (res + 1)^2 transposed-conv grid; per ToRGB the skip's Upsample (up 2, pad 2 / 1) and its
    adjoint (down 2)."""
    out = []
    for b in BATCHES:
        for res in (8, 16, 32, 64, 128, 256, 512, 1024):
            planes = b * CHANNELS[res]
            out += up_blur(planes, res, 1) + up_blur(planes, res, 0)
            out += [Q(planes, (res, res), (res + 1, res + 1), (4, 4), pad_x0=2),
                    Q(b * 3, (res // 2, res // 2), (res, res), (4, 4), up=2, pad_x0=2),
                    Q(b * 3, (res, res), (res // 2, res // 2), (4, 4), down=2, pad_x0=1)]
    return out


def discriminator_queries():
    """disc_hip.blur (pad 2, onto res + 1, in front of each stride-2 conv) and disc_hip.blur_adjoint (from the planar gradient)."""
    out = []
    for b in (2, 4):
        for res in (8, 16, 32, 64, 128, 256, 512, 1024):
            planes = b * CHANNELS[res]
            out += [Q(planes, (res, res), (res + 1, res + 1), (4, 4), pad_x0=2)] + up_blur(planes, res, 0)
    return out


SWEEP_OUT_W = (31, 32, 33, 255, 256, 257, 260)
SWEEP_TAPS = ((1, 1), (3, 3), (4, 4), (5, 3), (8, 8), (9, 9), (16, 16), (17, 3))


def sweep_queries():
    """The boundaries of the decision.  4x4 taps with up = down = 1, where every argument takes part: out_w x (in_w - out_w) x pad_x0 x
    layout x act x the two misalignments, in full.  The other tap shapes and up / down pairs, whose kernel depends on the taps, up,
    down, out_w, act and the layout alone: those, at in_w = out_w, pad 1, aligned."""
    out = []
    for ow, dw, pad, planar, act, xm, ym in itertools.product(SWEEP_OUT_W, (-1, 0, 1, 3, 8), (0, 1, 2, 3), (0, 1), (0, 1), (0, 4), (0, 4)):
        out.append(Q(6, (70, ow + dw), (70, ow), (4, 4), pad_x0=pad, planar=planar, act=act, xmis=xm, ymis=ym))
    for taps, up, down, ow, planar, act in itertools.product(SWEEP_TAPS, (1, 2, 3), (1, 2, 3), SWEEP_OUT_W, (0, 1), (0, 1)):
        out.append(Q(6, (70, ow), (70, ow), taps, up, down, 1, planar, act))
    return out


def limit_queries():
    """The size refusals and fall-throughs, each beside the nearest launch that passes; bad arguments; empty launches.  (The streaming
    kernel's own limit, 2^31 waves, cannot be reached through w2e_upfirdn2d: a launch has no more waves than tiles, and the tiles are
    counted first.  It is a refusal of the fused pass: actbwd_census.)"""
    big = 1 << 31
    return [
        Q(1 << 30, (64, 64), (64, 64), (3, 3), pad_x0=1), Q((1 << 30) - 1, (64, 64), (64, 64), (3, 3), pad_x0=1),      # n_tiles >= 2^31 (2 tiles per plane)
        Q(1 << 30, (64, 64), (64, 64), (4, 4), pad_x0=1), Q(1 << 29, (33, 257), (32, 256), (4, 4), pad_x0=1, planar=1),  # ... in front of blur4 / stream4
        Q(1, (46341, 46341), (64, 64), (3, 3)), Q(1, (46340, 46340), (64, 64), (3, 3)),                                   # in_h * in_w >= 2^31
        Q(1, (46341, 46341), (64, 256), (4, 4), pad_x0=2),
        Q(8, (8192, 8192), (4096, 4096), (4, 4), down=2, pad_x0=1), Q(8, (8192, 8191), (4096, 4095), (4, 4), down=2, pad_x0=1),  # down4: 2^29 input floats
        Q(1, (16, 16), (1 << 27, 16), (4, 4)), Q(1, (16, 16), ((1 << 27) - 1, 16), (4, 4)),                               # down4: 2^31 outputs
        Q(big, (16, 16), (16, 16), (4, 4), act=1), Q(big, (16, 16), (32, 32), (4, 4), up=2, pad_x0=2),                    # generic: a grid-stride loop, any size
        Q(2, (65, 65), (64, 64), (4, 4), pad_x0=1, planar=1, pitch=planar_pitch(32) + 4), Q(2, (65, 65), (64, 64), (4, 4), pad_x0=1, planar=1, pitch=36),
        Q(2, (33, 31), (32, 30), (4, 4), pad_x0=1, planar=1), Q(2, (17, 17), (16, 16), (4, 4), pad_x0=1, planar=1, act=1),  # planar, out_w < 32
        Q(2, (65, 65), (64, 64), (4, 4), pad_x0=1, planar=2), Q(2, (65, 65), (64, 64), (3, 3), pad_x0=1, planar=1),
        Q(2, (65, 65), (32, 32), (4, 4), down=2, pad_x0=1, planar=1), Q(2, (33, 33), (64, 64), (4, 4), up=2, pad_x0=2, planar=1),
        Q(-1, (8, 8), (8, 8), (4, 4)), Q(1, (0, 8), (8, 8), (4, 4)), Q(1, (8, 0), (8, 8), (4, 4)), Q(1, (8, 8), (-1, 8), (4, 4)), Q(1, (8, 8), (8, -1), (4, 4)),
        Q(1, (8, 8), (8, 8), (0, 4)), Q(1, (8, 8), (8, 8), (4, 17)), Q(1, (64, 64), (48, 62), (17, 3)),
        Q(1, (8, 8), (8, 8), (4, 4), up=0), Q(1, (8, 8), (8, 8), (4, 4), down=0),
        Q(0, (64, 64), (65, 65), (4, 4), pad_x0=2), Q(2, (64, 64), (0, 65), (4, 4), pad_x0=2), Q(2, (64, 64), (65, 0), (4, 4), pad_x0=2),
        Q(0, (65, 65), (64, 64), (4, 4), pad_x0=1, planar=1, pitch=7),                                                     # empty: returned before the layout is looked at
    ]


def fir_census():
    """[(origin, query)] in a fixed order, without repeated queries (the first origin keeps a repeated one)."""
    from test_gpu_fir_variants import FIR_MATRIX
    groups = (("matrix", [matrix_query(e) for e in FIR_MATRIX]), ("golden", golden_queries()), ("generator", generator_queries()),
              ("discriminator", discriminator_queries()), ("sweep", sweep_queries()), ("limits", limit_queries()))
    seen = {}
    for origin, queries in groups:
        for q in queries:
            seen.setdefault(q, origin)
    return [(origin, q) for q, origin in seen.items()]


def actbwd_census():
    """(planes, h, w, kh, kw) of w2e_blur_adjoint_actbwd_plan: ACTBWD_MATRIX, the activation backward of every up-sampling StyledConv of
    a step, the width rule's boundaries, other taps, and both sides of the plane and grid limits."""
    from test_gpu_fir_variants import ACTBWD_MATRIX
    out = [(n * c, h, w, 4, 4) for (n, c), h, w, _ in ACTBWD_MATRIX]
    out += [(b * CHANNELS[res], res, res, 4, 4) for b in BATCHES for res in (8, 16, 32, 64, 128, 256, 512, 1024)]
    out += [(6, 70, w, 4, 4) for w in (252, 255, 256, 257, 258, 260, 1023, 1024)]
    out += [(6, 70, 256, kh, kw) for kh, kw in ((3, 3), (4, 3), (3, 4), (5, 5), (1, 1))]
    out += [(0, 70, 256, 4, 4), (-1, 70, 256, 4, 4), (6, 0, 256, 4, 4),
            (1, 23170, 23168, 4, 4), (1, 23171, 23168, 4, 4),          # (h + 1) * (w + 1) against 2^29
            ((1 << 31) - 1, 1, 256, 4, 4), (1 << 31, 1, 256, 4, 4)]    # waves against 2^31
    return list(dict.fromkeys(out))


def option_sets():
    """([(name, options)] for w2e_upfirdn2d_plan, the same for w2e_blur_adjoint_actbwd_plan), each set written out in full."""
    full = lambda sets: [(name, dict(DEFAULT_OPTIONS, **o)) for name, o in sets]
    return (full([("default", {}), ("blur8", {"tune_blur": "8"})]),
            full([("default", {}), ("deterministic", {"deterministic": "1"}), ("fuse0", {"tune_fuse": "0"}), ("fuse1", {"tune_fuse": "1"})]))


def census():
    return [q for _, q in fir_census()], actbwd_census(), option_sets()


class Planner:
    """plan(query) -> [rc, message] for a refusal, else the FIELDS as a list; actbwd(query) -> 0 / 1; planar_ok(...) -> 0 / 1."""

    def __init__(self, lib):
        self.lib = lib
        lib.w2e_upfirdn2d_plan.restype = ctypes.c_int
        lib.w2e_upfirdn2d_plan.argtypes = [ctypes.c_int64] + [ctypes.c_int] * 14 + [ctypes.POINTER(ctypes.c_int64)]
        lib.w2e_blur_adjoint_actbwd_plan.restype = ctypes.c_int
        lib.w2e_blur_adjoint_actbwd_plan.argtypes = [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int)]
        lib.w2e_last_error.restype = ctypes.c_char_p
        lib.w2e_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]

    def set_options(self, options):
        for name, value in options.items():
            assert self.lib.w2e_set_option(name.encode(), value.encode()) == 0, name

    def plan(self, query):
        out = (ctypes.c_int64 * len(FIELDS))()
        rc = self.lib.w2e_upfirdn2d_plan(*query, out)
        return [rc, self.lib.w2e_last_error().decode()] if rc != 0 else list(out)

    def actbwd(self, query):
        fused = ctypes.c_int(-1)
        assert self.lib.w2e_blur_adjoint_actbwd_plan(*query, ctypes.byref(fused)) == 0
        return fused.value

    def planar_ok(self, kh, kw, up, down, out_w):
        self.lib.w2e_upfirdn2d_planar_ok.restype = ctypes.c_int
        self.lib.w2e_upfirdn2d_planar_ok.argtypes = [ctypes.c_int] * 5
        return self.lib.w2e_upfirdn2d_planar_ok(kh, kw, up, down, out_w)


def ask(planner, sets, queries, fn):
    """[[fn(query) per query] per option set], the options restored afterwards."""
    try:
        out = []
        for _, options in sets:
            planner.set_options(options)
            out.append([fn(q) for q in queries])
    finally:
        planner.set_options(DEFAULT_OPTIONS)
    return out


def record(planner):
    """The fixture: queries, option sets, the distinct results, and per option set the index of every query's result (upfirdn) or the
    answer itself (actbwd)."""
    queries, actbwd, (sets, actbwd_sets) = census()
    results, index, rows = [], {}, []
    for answers in ask(planner, sets, queries, planner.plan):
        row = []
        for r in answers:
            key = json.dumps(r)
            if key not in index:
                index[key] = len(results)
                results.append(r)
            row.append(index[key])
        rows.append(row)
    return {"fields": list(FIELDS), "queries": [list(q) for q in queries], "options": [[n, o] for n, o in sets], "results": results, "rows": rows,
            "actbwd_queries": [list(q) for q in actbwd], "actbwd_options": [[n, o] for n, o in actbwd_sets],
            "actbwd_rows": ask(planner, actbwd_sets, actbwd, planner.actbwd)}


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        from where2edit_amd import build
        path = build.build(verbose=False)
    fixture = record(Planner(ctypes.CDLL(path)))
    with open(OUT, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    n = len(fixture["queries"]) * len(fixture["options"]) + len(fixture["actbwd_queries"]) * len(fixture["actbwd_options"])
    print(f"{OUT}: {n} rows, {len(fixture['results'])} distinct results, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

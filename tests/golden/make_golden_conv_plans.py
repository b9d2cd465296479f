"""The census of conv-dispatcher decisions behind tests/golden/conv_plans.json (tests/test_conv_plan_host.py).

census() enumerates the queries -- shapes x option sets -- and record() asks a built library for the decision of each one: tile,
split-K, pipeline, LDS, grid and tile geometry (the fields of w2e_conv3x3_plan, include/w2e.h).  The test walks the same list through
the library under test and compares every field, so a refactor of the planner is shown on a CPU to have changed no decision.

The committed fixture was recorded from the commit BEFORE the planner became callable on its own (conv_impl, which planned and
launched in one function): a scratch copy of that commit with one exported function appended to modconv.hip that called conv_impl
with a ConvPlan (`use_all` added to it) and wrote the same fields out.  To re-record from a library that has w2e_conv3x3_plan:

    python tests/golden/make_golden_conv_plans.py [path/to/libw2e.so [symbol]]

Host code only: no GPU."""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "conv_plans.json")
FIELDS = ("use_all", "cfg", "splits", "k_per", "use_dma", "use_x3", "lds", "grid", "th", "tw", "tiles_x", "tiles_y", "tiles_n", "plane",
          "border_wgs")
SAME, UP, DOWN = 0, 1, 2
BENCH_SELECTIONS = os.path.join(ROOT, "profiles", "r05_bench_cfg_selections.txt")
IRSE_SHAPES = os.path.join(ROOT, "profiles", "r03_irse_shapes.txt")
# the planner's options, each set written out in full (value strings of w2e_set_option; "" = the library's own choice)
DEFAULT_OPTIONS = {"deterministic": "0", "conv_precision": "f32", "tune_dma": "", "tune_upall": "", "tune_cfg": ""}
LAYER_LINE = re.compile(r"modconv mode (\d)(?: \(all-phase\))? K (\d+) N (\d+) (\d+)x(\d+) B (\d+) -> cfg (\d+) splits (\d+)")


def bench_selections():
    """[(mode, k, n, h, w, b, cfg, split, dma)] of every direct conv launch in profiles/r05_bench_cfg_selections.txt."""
    out = []
    for ln in open(BENCH_SELECTIONS).read().splitlines():
        m = LAYER_LINE.match(ln)
        if m:
            mode, k, n, h, w, b, cfg, splits = (int(v) for v in m.groups())
            out.append([mode, k, n, h, w, b, cfg, splits > 1, False])
        elif ln.startswith("  lds-dma pipeline:") and out:
            out[-1][8] = ln.split(":")[1].strip().startswith("yes")
    return [tuple(r) for r in out]


def generator_layers(batch, size=1024):
    """The 3x3 convs of one StyleGAN2 step at `size`: forward (SAME; UP at the input resolution) and the input gradients (SAME with
    the channels swapped; DOWN for an up-sampling layer, h x w = its output)."""
    ch = {4: 512, 8: 512, 16: 512, 32: 512, 64: 512, 128: 256, 256: 128, 512: 64, 1024: 32}
    out = [(SAME, batch, 512, 512, 4, 4)]
    res, cin = 8, 512
    while res <= size:
        cout = ch[res]
        out += [(UP, batch, cin, cout, res // 2, res // 2), (DOWN, batch, cout, cin, res // 2, res // 2), (SAME, batch, cout, cout, res, res)]
        res, cin = 2 * res, cout
    return out


def shapes():
    """Every (mode, batch, k, n, h, w, prelu, down_pad) of the census, in a fixed order, without repeats."""
    from test_gpu_conv_variants import DIRECT_SHAPES
    out = []
    for mode, k, n, h, w, b, *_ in bench_selections():  # the benchmark's recorded launches; the record does not say which of them ran
        out.append((mode, b, k, n, h, w, 0, 0))        # with the bias / PReLU epilogue (the IR-SE50 ones): both
        if mode != UP:
            out.append((mode, b, k, n, h, w, 1, 0))
    for ln in open(IRSE_SHAPES).read().splitlines():  # IR-SE50 / e4e: "B16 64->128 56x56 ..."
        m = re.match(r"B(\d+) (\d+)->(\d+) (\d+)x(\d+)", ln)
        b, k, n, h, w = (int(v) for v in m.groups())
        out.append((SAME, b, k, n, h, w, 1, 0))
        out += [(DOWN, b, k, n, (h + 1) // 2, (w + 1) // 2, 1, pad) for pad in (0, 1)]  # the unit's stride-2 conv
    for name, mode in (("same", SAME), ("up", UP), ("down", DOWN)):
        b, k, n, h, w = DIRECT_SHAPES[name]
        out.append((mode, b, k, n, h, w, 0, 0))
    for batch in (1, 2, 16, 32):
        out += [s + (0, 0) for s in generator_layers(batch)]
    out += [  # edges: W < 32, W no power of two, K < 16, N = 3, an empty batch, a bad dimension, and both sides of the 4 GB limits
        (SAME, 2, 64, 64, 5, 7, 0, 0), (UP, 2, 64, 64, 5, 7, 0, 0), (DOWN, 2, 64, 64, 5, 7, 0, 0), (DOWN, 2, 64, 64, 5, 7, 1, 1),
        (SAME, 3, 48, 40, 33, 100, 0, 0), (UP, 3, 48, 40, 33, 100, 0, 0), (DOWN, 3, 48, 40, 33, 100, 0, 0), (SAME, 3, 48, 40, 33, 100, 1, 0),
        (SAME, 4, 3, 64, 112, 112, 0, 0), (UP, 4, 5, 16, 24, 24, 0, 0), (DOWN, 4, 9, 32, 48, 40, 0, 0),
        (SAME, 4, 64, 3, 112, 112, 0, 0), (UP, 4, 64, 3, 64, 64, 0, 0), (DOWN, 4, 64, 3, 64, 64, 0, 0), (SAME, 4, 64, 3, 112, 112, 1, 0),
        (SAME, 0, 64, 64, 32, 32, 0, 0), (SAME, 1, 0, 64, 32, 32, 0, 0), (UP, 1, 64, 64, 32, 32, 1, 0), (SAME, 1, 64, 64, 32, 32, 0, 1),
        (SAME, 1, 255, 32, 2048, 2048, 0, 0), (SAME, 1, 256, 32, 2048, 2048, 0, 0),   # input: 255 channels of 16 MB fit below 4 GB, 256 do not
        (SAME, 1, 32, 251, 2048, 2048, 0, 0), (SAME, 1, 32, 252, 2048, 2048, 0, 0),   # output: the limit less 16 planes of slack
        (UP, 1, 247, 16, 2048, 2048, 0, 0), (UP, 1, 248, 16, 2048, 2048, 0, 0),       # UP addresses channels up to K + 7
        (DOWN, 1, 63, 32, 2048, 2048, 0, 0), (DOWN, 1, 64, 32, 2048, 2048, 0, 0),     # DOWN reads a (2h + 1) x (2w + 1) image
    ]
    return list(dict.fromkeys(out))


def option_sets():
    """[(name, {option: value})]: the default, each planner option alone, and every tile forced with split requests 1 and 3 -- for
    every mode, and (third field of tune_cfg) for the UP launches only."""
    sets = [("default", {}), ("deterministic", {"deterministic": "1"}), ("bf16x3", {"conv_precision": "bf16x3"}),
            ("dma0", {"tune_dma": "0"}), ("dma1", {"tune_dma": "1"}), ("upall0", {"tune_upall": "0"}), ("upall1", {"tune_upall": "1"})]
    for cfg in range(12):
        for sp in (1, 3):
            sets.append((f"cfg{cfg}_s{sp}", {"tune_cfg": f"{cfg},{sp}"}))
        sets.append((f"cfg{cfg}_s3_up", {"tune_cfg": f"{cfg},3,{UP}"}))
    return [(name, dict(DEFAULT_OPTIONS, **o)) for name, o in sets]


def census():
    return shapes(), option_sets()


class Planner:
    """plan(shape) -> [rc, message] for a refusal, else the FIELDS as a list, from `symbol` of a loaded library."""

    def __init__(self, lib, symbol="w2e_conv3x3_plan"):
        self.lib = lib
        self.fn = getattr(lib, symbol)
        self.fn.restype = ctypes.c_int
        self.fn.argtypes = [ctypes.c_int] * 8 + [ctypes.POINTER(ctypes.c_int64)]
        lib.w2e_last_error.restype = ctypes.c_char_p
        lib.w2e_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]

    def set_options(self, options):
        for name, value in options.items():
            assert self.lib.w2e_set_option(name.encode(), value.encode()) == 0, name

    def plan(self, shape):
        out = (ctypes.c_int64 * len(FIELDS))()
        rc = self.fn(*shape, out)
        return [rc, self.lib.w2e_last_error().decode()] if rc != 0 else list(out)


def record(planner):
    """The fixture: shapes, option sets, the distinct results, and per option set the index of every shape's result."""
    shp, sets = census()
    results, index, rows = [], {}, []
    try:
        for _, options in sets:
            planner.set_options(options)
            row = []
            for s in shp:
                r = planner.plan(s)
                key = json.dumps(r)
                if key not in index:
                    index[key] = len(results)
                    results.append(r)
                row.append(index[key])
            rows.append(row)
    finally:
        planner.set_options(DEFAULT_OPTIONS)
    return {"fields": list(FIELDS), "shapes": [list(s) for s in shp], "options": [[n, o] for n, o in sets], "results": results, "rows": rows}


def main():
    if len(sys.argv) > 1:
        path = sys.argv[1]
    else:
        from where2edit_amd import build
        path = build.build(verbose=False)
    fixture = record(Planner(ctypes.CDLL(path), *sys.argv[2:3]))
    with open(OUT, "w") as f:
        json.dump(fixture, f, separators=(",", ":"))
        f.write("\n")
    print(f"{OUT}: {len(fixture['shapes'])} shapes x {len(fixture['options'])} option sets = "
          f"{len(fixture['shapes']) * len(fixture['options'])} rows, {len(fixture['results'])} distinct results, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

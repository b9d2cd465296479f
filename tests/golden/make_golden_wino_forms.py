"""The census of Winograd-form decisions behind tests/golden/wino_forms.json (tests/test_wino_plan_host.py).

Which form a stride-1 3x3 conv takes -- the direct kernel, the GEMM form (4) or the fused kernel (8) -- used to be decided in Python, by
functional._wino_form (the generator) and irse_hip._wino_form (the encoders) over functional._gemm_shape_ok / _fused_shape_ok, with the
GEMM form's tiles / K split / workspace from w2e_wino_gemm_plan plus four lines of arithmetic in functional.wino_gemm_conv for a forced
split.  All of that is now w2e_wino_plan (include/w2e.h).  The committed fixture was recorded from the LAST COMMIT THAT HAD THE PYTHON
FUNCTIONS, with _lib.get_option stubbed (the decisions need no library) and that commit's built w2e_wino_gemm_plan:

    python tests/golden/make_golden_wino_forms.py <checkout of that commit, built>

shapes() and groups() enumerate the queries; the test walks the same lists through the library under test.  The file is JSON: the grid
in the clear, the 645,120 recorded characters and the GEMM plans as the zlib-compressed JSON of PACKED, base64 in lines (load() undoes
it; in the clear it is 430 KB of digits).  Host code only: no GPU."""
import base64
import ctypes
import json
import os
import sys
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "wino_forms.json")

GENERATOR, ENCODER = 0, 1
EPI_PLAIN, EPI_DOT = 0, 3
FIELDS = ("form", "fits_gemm", "fits_fused", "tiles_padded", "splits", "workspace_floats")  # w2e_wino_plan's out[]

BATCHES = (1, 2, 4, 8, 16, 31, 32, 64, 127, 128)
CHANNELS = (3, 20, 32, 48, 64, 128, 256, 512)
SIZES = tuple((s, s) for s in (4, 7, 8, 14, 16, 28, 30, 32, 56, 64, 112, 128, 256, 512, 1024)) + (
    (16, 32), (32, 16), (30, 32), (64, 96), (256, 288), (2, 64))
# (name, family, epilogue, fused allowed): the two policies, each with the one switch its Python function had
VARIANTS = (("generator", GENERATOR, EPI_PLAIN, 1), ("generator_dot", GENERATOR, EPI_DOT, 1),
            ("encoder", ENCODER, EPI_PLAIN, 1), ("encoder_no_fused", ENCODER, EPI_PLAIN, 0))
REQUESTS = (("auto", -1), ("direct", 0), ("4", 4), ("8", 8))  # functional.WINOGRAD "auto" / False / 4 / 8
# (name, value strings of w2e_set_option, what w2e_get_option read back): only these two options enter the decision
OPTION_SETS = (("f32", {"conv_precision": "f32", "tune_cfg": ""}, {"conv_precision": 0, "tune_cfg": -1}),
               ("bf16x3", {"conv_precision": "bf16x3", "tune_cfg": ""}, {"conv_precision": 1, "tune_cfg": -1}),
               ("cfg3", {"conv_precision": "f32", "tune_cfg": "3"}, {"conv_precision": 0, "tune_cfg": 3}))
DEFAULT_OPTIONS = OPTION_SETS[0][1]
FORCED_SPLITS = (0, 2, 3, 8, 16)  # 0: the library's own K split


def shapes():
    """Every (batch, k, n, h, w) of the census, in a fixed order."""
    return [(b, k, n, h, w) for b in BATCHES for k in CHANNELS for n in CHANNELS for h, w in SIZES]


def groups():
    """[(key, variant, request, option set)]: one string of form digits per group, a character per shape."""
    return [(f"{v[0]}/{r[0]}/{o[0]}", v, r, o) for v in VARIANTS for r in REQUESTS for o in OPTION_SETS]


class Query:
    """w2e_wino_plan of a loaded library: plan(variant, request, shape, force_splits) -> the FIELDS as a list."""

    def __init__(self, lib):
        self.lib = lib
        lib.w2e_wino_plan.restype = ctypes.c_int
        lib.w2e_wino_plan.argtypes = [ctypes.c_int] * 10 + [ctypes.POINTER(ctypes.c_int64)]
        lib.w2e_last_error.restype = ctypes.c_char_p
        lib.w2e_set_option.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        self.out = (ctypes.c_int64 * len(FIELDS))()

    def set_options(self, options):
        for name, value in options.items():
            assert self.lib.w2e_set_option(name.encode(), value.encode()) == 0, name

    def plan(self, variant, request, shape, force_splits=0):
        _, family, epilogue, fused_allowed = variant
        rc = self.lib.w2e_wino_plan(family, request, fused_allowed, epilogue, *shape, force_splits, self.out)
        assert rc == 0, self.lib.w2e_last_error().decode()
        return list(self.out)


def record(root):
    """The fixture, from the Python policies and the w2e_wino_gemm_plan of the checkout at `root`."""
    sys.path.insert(0, root)
    from where2edit_amd import _lib, build, functional as K, irse_hip as I
    assert hasattr(K, "_gemm_shape_ok") and hasattr(K, "_fused_shape_ok"), f"{root} no longer decides in Python: record from the commit that did"
    lib = ctypes.CDLL(build.build(verbose=False))
    shp = shapes()
    strings, index = [], {}

    def intern(chars):
        s = "".join(chars)
        if s not in index:
            index[s] = len(strings)
            strings.append(s)
        return index[s]

    class X:  # functional._wino_form reads the batch off its tensors
        def __init__(self, b):
            self.shape = (b,)

    def form(variant, s):
        _, family, epilogue, fused_allowed = variant
        b, k, n, h, w = s
        if family == GENERATOR:
            return K._wino_form(X(b), k, n, h, w, X(b) if epilogue == EPI_DOT else None)
        I.FUSED_ENCODER = bool(fused_allowed)
        return I._wino_form(b, k, n, h, w)

    def fits(variant, s):  # (fits_gemm, fits_fused): each family's own arguments to the shape predicates
        b, k, n, h, w = s
        if variant[1] == GENERATOR:
            dot = variant[2] == EPI_DOT
            return K._gemm_shape_ok(b, k, n, h, w, dot), K._fused_shape_ok(b, k, n, h, w, dot)
        return K._gemm_shape_ok(b, k, n, h, w, dot=False, ragged=True), K._fused_shape_ok(b, k, n, h, w)

    saved = K.WINOGRAD, I.FUSED_ENCODER, _lib.get_option
    forms = {}
    try:
        for key, variant, (_, request), (_, _, read_back) in groups():
            _lib.get_option = read_back.__getitem__
            K.WINOGRAD = {-1: "auto", 0: False}.get(request, request)
            forms[key] = intern(str(form(variant, s)) for s in shp)
    finally:
        K.WINOGRAD, I.FUSED_ENCODER, _lib.get_option = saved
    flags = [[fits(v, s) for s in shp] for v in VARIANTS]
    fits_gemm = {v[0]: intern("01"[bool(f[0])] for f in fl) for v, fl in zip(VARIANTS, flags)}
    fits_fused = {v[0]: intern("01"[bool(f[1])] for f in fl) for v, fl in zip(VARIANTS, flags)}
    # the GEMM form's numbers, for every shape any group can answer 4 for (the encoders' predicate is the widest: ragged tiles, no dot)
    plans = []
    tp, sp, ws = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    for (b, k, n, h, w), f in zip(shp, flags[2]):
        if not f[0]:
            continue
        assert lib.w2e_wino_gemm_plan(b, k, n, h, w, ctypes.byref(tp), ctypes.byref(sp), ctypes.byref(ws)) == 0
        row = [tp.value]
        for forced in FORCED_SPLITS:
            splits, ws_floats = sp.value, ws.value
            if forced > 0 and forced != splits:  # functional.wino_gemm_conv's arithmetic for GEMM_SPLITS
                splits = min(forced, k // 8)
                kcs = -(-(k // 8) // splits)
                splits = -(-(k // 8) // kcs)
                ws_floats = b * n * max(1, -(-h // 4) * -(-w // 4) // 32) + (splits * b * n * h * w if splits > 1 else 0)
            row += [splits, ws_floats]
        plans.append(row)
    return {"batches": list(BATCHES), "channels": list(CHANNELS), "sizes": [list(s) for s in SIZES], "forced_splits": list(FORCED_SPLITS),
            "strings": strings, "forms": forms, "fits_gemm": fits_gemm, "fits_fused": fits_fused, "gemm_plans": plans}


PACKED = ("strings", "forms", "fits_gemm", "fits_fused", "gemm_plans")  # strings: the distinct form / fit strings the next three index


def load(path=OUT):
    """The fixture as record() returned it."""
    fixture = json.load(open(path))
    fixture.update(json.loads(zlib.decompress(base64.b64decode("".join(fixture.pop("packed"))))))
    return fixture


def main():
    fixture = record(os.path.abspath(sys.argv[1]))
    packed = base64.b64encode(zlib.compress(json.dumps({k: fixture.pop(k) for k in PACKED}, separators=(",", ":")).encode(), 9)).decode()
    fixture["packed"] = [packed[i:i + 120] for i in range(0, len(packed), 120)]
    with open(OUT, "w") as f:  # one key per line, the packed part one chunk per line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: " + (json.dumps(v) if k != "packed" else "[\n" + ",\n".join(map(json.dumps, v)) + "\n]")
                                   for k, v in fixture.items()) + "\n}\n")
    fixture = load()
    print(f"{OUT}: {len(shapes())} shapes x {len(groups())} groups = {len(shapes()) * len(groups())} decisions, "
          f"{len(fixture['strings'])} distinct strings, {len(fixture['gemm_plans'])} GEMM plans, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

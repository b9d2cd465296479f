"""The Inception-v3 feature extractor behind FID and the Inception Score (the network `torch_fidelity` runs for the reference's
`cal_evaluation`, utils.py:434-551), on the kernels of include/w2e_inception.h:

  * every one of the 94 `BasicConv2d` layers -- `relu(bn(conv(x)))`, BatchNorm in eval mode with eps = 1e-3 -- is one
    w2e_conv2d_bn_relu launch: BN is folded on the host, in float64, once, into a per-channel scale and shift (cached through
    derived.py), and each branch of a block writes its slice of the concatenated output, so no `cat` runs;
  * the pools are w2e_pool3x3 (max stride 2; the average that does not count padding; `Mixed_7c`'s stride-1 max pool -- the FID
    variant's quirk), B's and D's pooled branch landing in its slice as well;
  * the input is w2e_inception_resize: uint8 [B,H,W,3] of any size -> the legacy-TensorFlow bilinear resize to 299 x 299 and
    (v - 128) / 128, one launch;
  * the global means are w2e_channel_sums, the `fc` head is the same convolution kernel on [B,2048,1,1] with the identity
    activation.

Weights: the parameter names are those of torch_fidelity's `pt_inception-2015-12-05` checkpoint (`NAME.conv.weight`,
`NAME.bn.{weight,bias,running_mean,running_var}`, `fc.weight`, `fc.bias`: 94 * 5 + 2 = 472 tensors; `num_batches_tracked` is accepted
and ignored), so `load_state_dict` takes the published file.  Without a file the network keeps a SEEDED RANDOM initialisation
(He-normal convolutions, identity BatchNorm) -- for synthetic benchmarking and tests, as Vgg16 and CLIP do: there is no network to
fetch the pretrained file from, and the features of a random network are no Inception features.

The definition is restated from the published architecture; it could not be compared against torch_fidelity or torchvision
themselves (DESIGN.md "K18").  A frozen, forward-only critic: a parameter that requires grad is refused, there is no stock-op
fallback and no host synchronisation in forward."""
import torch

from ._lib import CONSTS, call, ptr, stream_ptr
from .derived import derived

SIZE = CONSTS["W2E_INCEPTION_SIZE"]
POOL_MAX_S2, POOL_AVG, POOL_MAX_S1 = CONSTS["W2E_POOL_MAX_S2"], CONSTS["W2E_POOL_AVG_S1P1"], CONSTS["W2E_POOL_MAX_S1P1"]
BN_EPS = 1e-3
FEATURES = ("768", "2048", "logits_unbiased", "logits")


def _conv(name, cin, cout, k=1, stride=1, pad=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    return (name, cin, cout, kh, kw, stride, ph, pw)


def _a(n, cin, pf):
    return [_conv(f"{n}.branch1x1", cin, 64), _conv(f"{n}.branch5x5_1", cin, 48), _conv(f"{n}.branch5x5_2", 48, 64, 5, pad=2),
            _conv(f"{n}.branch3x3dbl_1", cin, 64), _conv(f"{n}.branch3x3dbl_2", 64, 96, 3, pad=1), _conv(f"{n}.branch3x3dbl_3", 96, 96, 3, pad=1),
            _conv(f"{n}.branch_pool", cin, pf)]


def _b(n, cin):
    return [_conv(f"{n}.branch3x3", cin, 384, 3, stride=2), _conv(f"{n}.branch3x3dbl_1", cin, 64), _conv(f"{n}.branch3x3dbl_2", 64, 96, 3, pad=1),
            _conv(f"{n}.branch3x3dbl_3", 96, 96, 3, stride=2)]


def _c(n, c7):
    row, col = dict(k=(1, 7), pad=(0, 3)), dict(k=(7, 1), pad=(3, 0))
    return [_conv(f"{n}.branch1x1", 768, 192), _conv(f"{n}.branch7x7_1", 768, c7), _conv(f"{n}.branch7x7_2", c7, c7, **row),
            _conv(f"{n}.branch7x7_3", c7, 192, **col), _conv(f"{n}.branch7x7dbl_1", 768, c7), _conv(f"{n}.branch7x7dbl_2", c7, c7, **col),
            _conv(f"{n}.branch7x7dbl_3", c7, c7, **row), _conv(f"{n}.branch7x7dbl_4", c7, c7, **col), _conv(f"{n}.branch7x7dbl_5", c7, 192, **row),
            _conv(f"{n}.branch_pool", 768, 192)]


def _d(n):
    return [_conv(f"{n}.branch3x3_1", 768, 192), _conv(f"{n}.branch3x3_2", 192, 320, 3, stride=2), _conv(f"{n}.branch7x7x3_1", 768, 192),
            _conv(f"{n}.branch7x7x3_2", 192, 192, (1, 7), pad=(0, 3)), _conv(f"{n}.branch7x7x3_3", 192, 192, (7, 1), pad=(3, 0)),
            _conv(f"{n}.branch7x7x3_4", 192, 192, 3, stride=2)]


def _e(n, cin):
    row, col = dict(k=(1, 3), pad=(0, 1)), dict(k=(3, 1), pad=(1, 0))
    return [_conv(f"{n}.branch1x1", cin, 320), _conv(f"{n}.branch3x3_1", cin, 384), _conv(f"{n}.branch3x3_2a", 384, 384, **row),
            _conv(f"{n}.branch3x3_2b", 384, 384, **col), _conv(f"{n}.branch3x3dbl_1", cin, 448), _conv(f"{n}.branch3x3dbl_2", 448, 384, 3, pad=1),
            _conv(f"{n}.branch3x3dbl_3a", 384, 384, **row), _conv(f"{n}.branch3x3dbl_3b", 384, 384, **col), _conv(f"{n}.branch_pool", cin, 192)]


# (block name, kind, pool of its branch_pool) in network order; the stem's five convolutions come first in LAYERS
BLOCKS = (("Mixed_5b", "A"), ("Mixed_5c", "A"), ("Mixed_5d", "A"), ("Mixed_6a", "B"), ("Mixed_6b", "C"), ("Mixed_6c", "C"),
          ("Mixed_6d", "C"), ("Mixed_6e", "C"), ("Mixed_7a", "D"), ("Mixed_7b", "E"), ("Mixed_7c", "E"))
E_POOL = {"Mixed_7b": POOL_AVG, "Mixed_7c": POOL_MAX_S1}
# every BasicConv2d: (name, cin, cout, kh, kw, stride, ph, pw)
LAYERS = tuple(
    [_conv("Conv2d_1a_3x3", 3, 32, 3, stride=2), _conv("Conv2d_2a_3x3", 32, 32, 3), _conv("Conv2d_2b_3x3", 32, 64, 3, pad=1),
     _conv("Conv2d_3b_1x1", 64, 80), _conv("Conv2d_4a_3x3", 80, 192, 3)]
    + _a("Mixed_5b", 192, 32) + _a("Mixed_5c", 256, 64) + _a("Mixed_5d", 288, 64) + _b("Mixed_6a", 288)
    + _c("Mixed_6b", 128) + _c("Mixed_6c", 160) + _c("Mixed_6d", 160) + _c("Mixed_6e", 192) + _d("Mixed_7a")
    + _e("Mixed_7b", 1280) + _e("Mixed_7c", 2048))
SPEC = {layer[0]: layer for layer in LAYERS}
FC = (1008, 2048)


def state_dict_shapes():
    """{key: shape} of the 472 tensors of the checkpoint."""
    shapes = {}
    for name, cin, cout, kh, kw, _, _, _ in LAYERS:
        shapes[f"{name}.conv.weight"] = (cout, cin, kh, kw)
        for kind in ("weight", "bias", "running_mean", "running_var"):
            shapes[f"{name}.bn.{kind}"] = (cout,)
    shapes["fc.weight"], shapes["fc.bias"] = FC, (FC[0],)
    return shapes


class _Conv(torch.nn.Module):
    def __init__(self, shape):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(shape), requires_grad=False)


class _BatchNorm(torch.nn.Module):
    """The four tensors of an eval-mode BatchNorm2d (no num_batches_tracked: nothing here trains)."""

    def __init__(self, channels):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(channels), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(channels), requires_grad=False)
        self.register_buffer("running_mean", torch.zeros(channels))
        self.register_buffer("running_var", torch.ones(channels))


class BasicConv2d(torch.nn.Module):
    def __init__(self, cin, cout, kh, kw):
        super().__init__()
        self.conv = _Conv((cout, cin, kh, kw))
        self.bn = _BatchNorm(cout)


class _Linear(torch.nn.Module):
    def __init__(self, out_features, in_features):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.empty(out_features, in_features), requires_grad=False)
        self.bias = torch.nn.Parameter(torch.zeros(out_features), requires_grad=False)


def fold_bn(weight, bias, mean, var, eps=BN_EPS):
    """Eval-mode BatchNorm as y = scale * x + shift per channel, computed in float64 and rounded once to fp32."""
    scale = weight.double() / torch.sqrt(var.double() + eps)
    return scale.float(), (bias.double() - mean.double() * scale).float()


class _Plan:
    """Per layer: the weight as the kernel reads it (OIHW, fp32, contiguous) and the folded BatchNorm."""

    def __init__(self, net):
        self.w, self.scale, self.shift = {}, {}, {}
        with torch.no_grad():
            for name, *_ in LAYERS:
                m = net.get_submodule(name)
                self.w[name] = m.conv.weight.detach().float().contiguous()
                self.scale[name], self.shift[name] = (t.contiguous() for t in fold_bn(m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var))
            self.fc_w = net.fc.weight.detach().float().contiguous().view(FC[0], FC[1], 1, 1)
            self.fc_b = net.fc.bias.detach().float().contiguous()
        # the layers' constant arguments as the call takes them, made once (the tensors above keep the addresses alive): 94 launches
        # per forward, and at batch 1 the host is as long on them as the device
        self.args = {}
        if self.fc_b.is_cuda:
            for name, cin, cout, kh, kw, stride, ph, pw in LAYERS:
                self.args[name] = (ptr(self.w[name]), ptr(self.scale[name]), ptr(self.shift[name]))


# ---------------------------------------------------------------------------------------------- raw kernel calls
def conv2d_bn_relu(x, w, scale, shift, stride=1, padding=(0, 0), relu=True, out=None, ch_off=0):
    """w2e_conv2d_bn_relu: x [B,Cin,H,W], w [N,Cin,KH,KW]; the result goes to channels [ch_off, ch_off + N) of `out` (allocated with N
    channels when None).  Returns `out`."""
    b, cin, h, wd = x.shape
    n, cin_w, kh, kw = w.shape
    if cin_w != cin:
        raise RuntimeError(f"conv2d_bn_relu: x has {cin} channels, the weight takes {cin_w}")
    ph, pw = padding
    oh, ow = (h + 2 * ph - kh) // stride + 1, (wd + 2 * pw - kw) // stride + 1
    if out is None:
        out = torch.empty((b, n, oh, ow), device=x.device, dtype=torch.float32)
    elif out.shape[0] != b or tuple(out.shape[2:]) != (oh, ow):
        raise RuntimeError(f"conv2d_bn_relu: the output is {tuple(out.shape)}, the result [{b}, {n}, {oh}, {ow}]")
    call("w2e_conv2d_bn_relu", ptr(x), ptr(w), ptr(scale), ptr(shift), ptr(out), b, cin, h, wd, n, kh, kw, stride, ph, pw, int(relu),
         out.shape[1], ch_off, stream_ptr())
    return out


def pool3x3(x, mode, out=None, ch_off=0):
    """w2e_pool3x3 into channels [ch_off, ch_off + C) of `out` (allocated with C channels when None)."""
    b, c, h, w = x.shape
    oh, ow = ((h - 3) // 2 + 1, (w - 3) // 2 + 1) if mode == POOL_MAX_S2 else (h, w)
    if out is None:
        out = torch.empty((b, c, oh, ow), device=x.device, dtype=torch.float32)
    elif out.shape[0] != b or tuple(out.shape[2:]) != (oh, ow):
        raise RuntimeError(f"pool3x3: the output is {tuple(out.shape)}, the result [{b}, {c}, {oh}, {ow}]")
    call("w2e_pool3x3", ptr(x), ptr(out), b, c, h, w, mode, out.shape[1], ch_off, stream_ptr())
    return out


def resize_input(x):
    """w2e_inception_resize: uint8 [B,H,W,3] on the GPU -> fp32 [B,3,299,299]."""
    if not (x.is_cuda and x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] == 3):
        raise RuntimeError(f"FeatureExtractorInceptionV3: images are uint8 [B,H,W,3] on the GPU (got {x.dtype} {tuple(x.shape)} on {x.device})")
    if x.device.index != torch.cuda.current_device():
        raise RuntimeError(f"FeatureExtractorInceptionV3: images on {x.device} but the current device is cuda:{torch.cuda.current_device()}")
    x = x if x.is_contiguous() else x.contiguous()
    b, h, w, _ = x.shape
    out = torch.empty((b, 3, SIZE, SIZE), device=x.device, dtype=torch.float32)
    import ctypes
    call("w2e_inception_resize", ctypes.c_void_p(x.data_ptr() if b else 16), ptr(out), b, h, w, stream_ptr())
    return out


def spatial_mean(x):
    """[B,C,H,W] -> [B,C]: w2e_channel_sums times 1 / (H W)."""
    b, c, h, w = x.shape
    sums = torch.empty((b, c), device=x.device, dtype=torch.float32)
    call("w2e_channel_sums", ptr(x), None, ptr(sums), b, c, h * w, stream_ptr())
    return sums * (1.0 / (h * w))


class FeatureExtractorInceptionV3(torch.nn.Module):
    """torch_fidelity's `FeatureExtractorInceptionV3` (the `pt_inception-2015-12-05` FID network) on the kernels above.
    `forward(x, features=('2048', 'logits_unbiased'))`: x uint8 [B,H,W,3] on the GPU (what the decoders and
    `to_bytes(grid=False)` return) -> a tuple of the named features, in that order: '768' (Mixed_6e averaged over 17 x 17), '2048' (the
    mean over 8 x 8), 'logits_unbiased' (f @ fc.weight.T) and 'logits' (+ fc.bias).
    Without loaded weights the network holds a seeded RANDOM initialisation: its numbers are then no FID / IS of the literature."""

    def __init__(self, seed=0):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for name, cin, cout, kh, kw, _, _, _ in LAYERS:
            parent = self
            *path, leaf = name.split(".")
            for part in path:
                if not hasattr(parent, part):
                    parent.add_module(part, torch.nn.Module())
                parent = getattr(parent, part)
            m = BasicConv2d(cin, cout, kh, kw)
            m.conv.weight.data.normal_(0.0, (2.0 / (cin * kh * kw)) ** 0.5, generator=g)
            parent.add_module(leaf, m)
        self.fc = _Linear(*FC)
        self.fc.weight.data.normal_(0.0, FC[1] ** -0.5, generator=g)

    def load_state_dict(self, state_dict, strict=True, **kw):
        """The checkpoint's 472 tensors; `*.num_batches_tracked` entries are dropped.  A missing or misshapen tensor raises with its
        key."""
        sd = {k: v for k, v in state_dict.items() if not k.endswith(".num_batches_tracked")}
        for key, shape in state_dict_shapes().items():
            if key not in sd:
                if strict:
                    raise KeyError(f"Inception-v3 weights: no tensor for {key}")
            elif tuple(sd[key].shape) != shape:
                raise RuntimeError(f"Inception-v3 weights: {key} has shape {tuple(sd[key].shape)}, expected {shape}")
        return super().load_state_dict(sd, strict=strict, **kw)

    def plan(self):
        """The folded parameters (cached: derived.py)."""
        return derived(self, "_plan", list(self.parameters()) + list(self.buffers()), lambda: _Plan(self))

    def _refuse_trainable(self):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise RuntimeError("where2edit_amd: an Inception-v3 parameter requires grad.  The HIP kernels run the network as a frozen, "
                               "forward-only critic (there is no backward and no stock-op fallback): call .requires_grad_(False) on it.")

    # ------------------------------------------------------------------------------------------ the layers
    def _cv(self, P, name, x, out=None, ch_off=0):
        """conv2d_bn_relu for a layer of the network, with its constant arguments from the plan."""
        _, cin_w, cout, kh, kw, stride, ph, pw = SPEC[name]
        weight, scale, shift = P.args[name]
        b, cin, h, w = x.shape
        if cin != cin_w:
            raise RuntimeError(f"{name}: the input has {cin} channels, the layer takes {cin_w}")
        oh, ow = (h + 2 * ph - kh) // stride + 1, (w + 2 * pw - kw) // stride + 1
        if out is None:
            out = torch.empty((b, cout, oh, ow), device=x.device, dtype=torch.float32)
        elif out.shape[0] != b or tuple(out.shape[2:]) != (oh, ow):
            raise RuntimeError(f"{name}: the output is {tuple(out.shape)}, the result [{b}, {cout}, {oh}, {ow}]")
        call("w2e_conv2d_bn_relu", ptr(x), weight, scale, shift, ptr(out), b, cin, h, w, cout, kh, kw, stride, ph, pw, 1, out.shape[1], ch_off, stream_ptr())
        return out

    def stem(self, x, P=None):
        """fp32 [B,3,299,299] -> [B,192,35,35]."""
        P = P or self.plan()
        x = self._cv(P, "Conv2d_1a_3x3", x)
        x = self._cv(P, "Conv2d_2a_3x3", x)
        x = self._cv(P, "Conv2d_2b_3x3", x)
        x = pool3x3(x, POOL_MAX_S2)
        x = self._cv(P, "Conv2d_3b_1x1", x)
        x = self._cv(P, "Conv2d_4a_3x3", x)
        return pool3x3(x, POOL_MAX_S2)

    def block(self, name, x, P=None):
        """One Mixed_* block on fp32 [B,C,H,W] of any spatial size its windows fit in."""
        P = P or self.plan()
        kind = dict(BLOCKS)[name]
        b, c, h, w = x.shape
        cv = lambda leaf, t, out=None, off=0: self._cv(P, f"{name}.{leaf}", t, out, off)
        width = lambda *leaves: sum(SPEC[f"{name}.{leaf}"][2] for leaf in leaves)
        new = lambda ch, oh, ow: torch.empty((b, ch, oh, ow), device=x.device, dtype=torch.float32)
        if kind == "A":
            y = new(width("branch1x1", "branch5x5_2", "branch3x3dbl_3", "branch_pool"), h, w)
            cv("branch1x1", x, y, 0)
            cv("branch5x5_2", cv("branch5x5_1", x), y, 64)
            cv("branch3x3dbl_3", cv("branch3x3dbl_2", cv("branch3x3dbl_1", x)), y, 128)
            cv("branch_pool", pool3x3(x, POOL_AVG), y, 224)
        elif kind == "B":
            oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            y = new(384 + 96 + c, oh, ow)
            cv("branch3x3", x, y, 0)
            cv("branch3x3dbl_3", cv("branch3x3dbl_2", cv("branch3x3dbl_1", x)), y, 384)
            pool3x3(x, POOL_MAX_S2, y, 480)
        elif kind == "C":
            y = new(768, h, w)
            cv("branch1x1", x, y, 0)
            cv("branch7x7_3", cv("branch7x7_2", cv("branch7x7_1", x)), y, 192)
            t = cv("branch7x7dbl_1", x)
            for leaf in ("branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4"):
                t = cv(leaf, t)
            cv("branch7x7dbl_5", t, y, 384)
            cv("branch_pool", pool3x3(x, POOL_AVG), y, 576)
        elif kind == "D":
            oh, ow = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            y = new(320 + 192 + c, oh, ow)
            cv("branch3x3_2", cv("branch3x3_1", x), y, 0)
            t = cv("branch7x7x3_1", x)
            for leaf in ("branch7x7x3_2", "branch7x7x3_3"):
                t = cv(leaf, t)
            cv("branch7x7x3_4", t, y, 320)
            pool3x3(x, POOL_MAX_S2, y, 512)
        else:
            y = new(2048, h, w)
            cv("branch1x1", x, y, 0)
            t = cv("branch3x3_1", x)
            cv("branch3x3_2a", t, y, 320)
            cv("branch3x3_2b", t, y, 704)
            t = cv("branch3x3dbl_2", cv("branch3x3dbl_1", x))
            cv("branch3x3dbl_3a", t, y, 1088)
            cv("branch3x3dbl_3b", t, y, 1472)
            cv("branch_pool", pool3x3(x, E_POOL[name]), y, 1856)
        return y

    def forward(self, x, features=("2048", "logits_unbiased")):
        self._refuse_trainable()
        for f in features:
            if f not in FEATURES:
                raise ValueError(f"FeatureExtractorInceptionV3: unknown feature {f!r}; the features are {FEATURES}")
        P = self.plan()
        if P.fc_b.device != x.device:
            raise RuntimeError(f"FeatureExtractorInceptionV3: the weights are on {P.fc_b.device}, the images on {x.device}")
        out = {}
        with torch.no_grad():
            h = self.stem(resize_input(x), P)
            for name, _ in BLOCKS:
                h = self.block(name, h, P)
                if name == "Mixed_6e" and "768" in features:
                    out["768"] = spatial_mean(h)
            f = spatial_mean(h)
            out["2048"] = f
            f4 = f.view(f.shape[0], FC[1], 1, 1)
            if "logits_unbiased" in features:
                out["logits_unbiased"] = conv2d_bn_relu(f4, P.fc_w, None, None, relu=False).view(-1, FC[0])
            if "logits" in features:
                out["logits"] = conv2d_bn_relu(f4, P.fc_w, None, P.fc_b, relu=False).view(-1, FC[0])
        return tuple(out[f] for f in features)

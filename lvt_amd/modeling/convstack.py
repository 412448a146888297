"""Shared machinery of the conv encoder / decoder modules: the autograd node that runs a whole conv
stack on the HIP engine, and the boundary layout conversion."""
import torch
from torch import nn

from ..hip import binding as L
from ..hip import convnet, ew


class _ConvStackFn(torch.autograd.Function):
    """forward(x_cl, layers, layers_grad, norms, *params) -> y_cl.  One autograd node per sub-network: the backward runs
    the hand-scheduled chain of lvt_amd.hip.convnet.stack_backward and hands all parameter gradients back at once.
    params: (weight, bias) of every layer (bias None where the layer is normalised), then (gamma, beta) of every layer
    with trainable batch normalisation."""

    @staticmethod
    def forward(ctx, x, layers, layers_grad, norms, *flat):
        # layers_grad: torch.is_grad_enabled() at the CALL site (inside forward autograd has already switched it off, and
        # needs_input_grad is True for parameters even under torch.no_grad()): eval passes skip the backward weight layouts
        params = [(flat[2 * i], flat[2 * i + 1]) for i in range(len(layers))]
        with torch.no_grad():
            outs, saved = convnet.stack_forward(layers, x, params, want_grad=layers_grad and any(ctx.needs_input_grad),
                                                norms=norms)
        ctx.layers, ctx.saved, ctx.outs, ctx.x = layers, saved, outs, x
        ctx.shapes = [tuple(p.shape) if p is not None else None for p in flat]
        return outs[-1]

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        with torch.no_grad():
            gx, grads, norm_grads = convnet.stack_backward(ctx.layers, ctx.x, ctx.outs, ctx.saved, gy,
                                                           need_input_grad=ctx.needs_input_grad[0])
        flat = []
        for i, (dw, db) in enumerate(grads):
            flat.append(dw.view(ctx.shapes[2 * i]) if dw is not None else None)        # (None: a pool / upsample layer)
            flat.append(db.contiguous().view(ctx.shapes[2 * i + 1]) if db is not None else None)
        for dgamma, dbeta in norm_grads:
            flat += [dgamma, dbeta]
        ctx.outs = ctx.saved = None
        return (gx, None, None, None) + tuple(flat)


def run_stack(x_cl, layers, params, norms=None):
    """params: [(weight, bias or None)] per layer.  norms: the normalisation module of every layer (None where it has
    none); their train / eval state picks batch statistics, running statistics or the eval fold."""
    flat = [t for wb in params for t in wb]
    if norms is not None:
        flat += [t for ly, m in zip(layers, norms) if ly.norm in ("bn", "syncbn") for t in (m.weight, m.bias)]
    return _ConvStackFn.apply(x_cl, layers, torch.is_grad_enabled(), norms, *flat)


def nchw_to_cl(x, cpad=None):
    """(N,C,H,W) -> (N,1,H,W,Cp) channels-last, channels zero-padded to a multiple of 4."""
    L.require(x)
    n, c, h, w = x.shape
    cp = cpad or (c + 3) // 4 * 4
    return ew.to_channels_last(x.reshape(n, c, h * w), cp).view(n, 1, h, w, cp)


def cl_to_nchw(y, c):
    """(N,1,H,W,Cp) -> (N,C,H,W)."""
    n, _, h, w, cp = y.shape
    return ew.to_channels_first(y.view(n, h * w, cp), c).view(n, c, h, w)


class _LayoutIn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.c = x.shape[1]
        return nchw_to_cl(x.contiguous())

    @staticmethod
    def backward(ctx, g):
        return cl_to_nchw(g.contiguous(), ctx.c)


class _LayoutOut(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, c):
        ctx.cp = y.shape[-1]
        return cl_to_nchw(y, c)

    @staticmethod
    def backward(ctx, g):
        return nchw_to_cl(g.contiguous(), ctx.cp), None


SUPPORTED_NORMS = ("", "BN", "SyncBN", "FrozenBN")
_OUT_ACTIVATIONS = {"": None, "sigmoid": nn.Sigmoid, "tanh": nn.Tanh}


def out_activation_module(name):
    """The module the reference appends as the last child of `layers` for OUT_ACTIVATION `name` (None for ""; it has no
    state-dict keys), or ValueError for a string the reference does not know either."""
    if name not in _OUT_ACTIVATIONS:
        raise ValueError("Unknown activation %r" % (name,))
    cls = _OUT_ACTIVATIONS[name]
    return cls() if cls is not None else None


def act_after(nxt):
    """Activation the plan folds into the layer whose output the module `nxt` consumes: an explicit ReLU or a ResBlock
    (whose first op is an in-place ReLU) rectifies it, a LeakyReLU(0.2) does so with its slope, a trailing Tanh / Sigmoid is
    the stack's output activation."""
    if isinstance(nxt, (nn.ReLU, ResBlock)):
        return "relu"
    if isinstance(nxt, nn.LeakyReLU):
        if nxt.negative_slope != 0.2:
            raise NotImplementedError("LeakyReLU slope %r: the kernels implement 0.2 only" % (nxt.negative_slope,))
        return "leaky"
    if isinstance(nxt, nn.Tanh):
        return "tanh"
    if isinstance(nxt, nn.Sigmoid):
        return "sigmoid"
    return ""


def check_norm(norm, spectral):
    if (norm or "") not in SUPPORTED_NORMS or spectral:
        raise NotImplementedError("lvt_amd implements NORM in {%s} without spectral norm for ResEncoder / ResDecoder; got "
                                  "norm=%r spectral=%r" % (", ".join(repr(n) for n in SUPPORTED_NORMS), norm, spectral))


class NaiveSyncBatchNorm(nn.BatchNorm2d):
    """The reference's cross-rank BatchNorm (vidgen/layers/batch_norm.py, stats_mode ""): the parameters, buffers and
    state-dict keys of nn.BatchNorm2d.  A parameter container: the conv stack computes it (hip/convnet.py).  At world
    size > 1 in train mode the mean and E[x^2] are equal-weight averages over the ranks, running_var receives the biased
    variance and num_batches_tracked stays; otherwise it is nn.BatchNorm2d."""

    def __init__(self, *args, stats_mode="", **kwargs):
        super().__init__(*args, **kwargs)
        if stats_mode != "":
            raise NotImplementedError("NaiveSyncBatchNorm: only stats_mode '' is implemented")
        self._stats_mode = stats_mode


class FrozenBatchNorm2d(nn.Module):
    """FrozenBN: a per-channel affine map built from fixed statistics, with the reference's checkpoint contract -- four
    buffers (`weight`, `bias`, `running_mean`, `running_var`), no parameters, state-dict version 3.  It starts as the
    identity: `running_var` holds 1 - eps, because the map adds eps back.  A parameter container, as above."""

    _version = 3

    def __init__(self, num_features, eps=1e-5):
        super().__init__()
        self.num_features, self.eps = num_features, eps
        identity = {"weight": torch.ones(num_features), "bias": torch.zeros(num_features),
                    "running_mean": torch.zeros(num_features), "running_var": torch.ones(num_features) - eps}
        for name, t in identity.items():
            self.register_buffer(name, t)

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, *args):
        saved = local_metadata.get("version")
        old = saved is None or saved < 2
        for name in ("running_mean", "running_var"):
            if old and prefix + name not in state_dict:
                # checkpoints older than version 2 carry no statistics: keep the identity (var 1 before the shift below)
                state_dict[prefix + name] = torch.zeros_like(self.running_mean) if name == "running_mean" \
                    else torch.ones_like(self.running_var)
        if saved is not None and saved < 3:
            # version 2 stored the variance with eps included
            state_dict[prefix + "running_var"] = state_dict[prefix + "running_var"] - self.eps
        super()._load_from_state_dict(state_dict, prefix, local_metadata, *args)

    def extra_repr(self):
        return "%d, eps=%g" % (self.num_features, self.eps)


_NORM_MODULES = {"BN": nn.BatchNorm2d, "SyncBN": NaiveSyncBatchNorm, "FrozenBN": FrozenBatchNorm2d}


def norm_layer(layer, norm):
    """The reference's wrapper (vidgen/layers/wrappers.py norm_layer): a normalised conv loses its bias and becomes
    Sequential(conv, norm)."""
    if norm:
        layer.bias = None           # the norm's shift makes a conv bias redundant; the key is unregistered, not kept
        layer = nn.Sequential(layer, _NORM_MODULES[norm](layer.out_channels))
    return layer


def split_norm(m):
    """A conv or Sequential(conv, norm) -> (conv, norm module or None, the plan's norm kind)."""
    if isinstance(m, nn.Sequential):
        conv, nm = m[0], m[1]
        kind = "frozen" if isinstance(nm, FrozenBatchNorm2d) else "syncbn" if isinstance(nm, NaiveSyncBatchNorm) else "bn"
        return conv, nm, kind
    return m, None, ""


def is_conv(m, cls):
    """m is a `cls` layer, plain or normalised."""
    return isinstance(m, cls) or (isinstance(m, nn.Sequential) and len(m) == 2 and isinstance(m[0], cls))


def plain_plan(layers):
    """Plan of a Sequential of 3x3-style convolutions (plain or normalised), LeakyReLU / ReLU, AvgPool2d(2), Upsample(2) and an
    optional output activation -- the ConvEncoder / ConvDecoder families.  -> (plan, owners, norms): one convnet.Layer per conv,
    pool and upsample; owners[i] the conv module of layer i (None for a pool / upsample), norms as run_stack takes them."""
    Layer = convnet.Layer
    mods = list(layers)
    plan, owners, norms = [], [], []
    for i, m in enumerate(mods):
        nxt = mods[i + 1] if i + 1 < len(mods) else None
        if is_conv(m, nn.Conv2d):
            conv, nm, kind = split_norm(m)
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            plan.append(Layer("conv", (1, k, k), (1, s, s), (0, p, p), conv.in_channels, conv.out_channels,
                              act=act_after(nxt), norm=kind))
            owners.append(conv)
            norms.append(nm)
        elif isinstance(m, (nn.AvgPool2d, nn.Upsample)):
            if isinstance(m, nn.AvgPool2d):
                ok, kind = m.kernel_size == 2 and m.stride == 2 and m.padding == 0, "pool"
            else:
                ok, kind = m.scale_factor == 2 and m.mode == "nearest" and m.size is None, "up"
            if not ok or not plan:
                raise NotImplementedError("only AvgPool2d(2) / nearest Upsample(scale_factor=2) behind a convolution: %r" % (m,))
            plan.append(Layer.resample(kind, plan[-1].cout))
            owners.append(None)
            norms.append(None)
        elif not isinstance(m, (nn.LeakyReLU, nn.ReLU, nn.Tanh, nn.Sigmoid)):
            raise NotImplementedError("no plan for %r" % (m,))
    return plan, owners, (norms if any(n is not None for n in norms) else None)


def plan_params(owners):
    """[(weight, bias)] of a plan's layers for run_stack; (None, None) for the parameter-less ones."""
    return [(m.weight, m.bias) if m is not None else (None, None) for m in owners]


class ResBlock(nn.Module):
    """Parameter container with the reference's key names (`block.1`, `block.3`; `block.1.0`, `block.1.1` when
    normalised); resencoder.py:10-21 / resdecoder.py:10-21, whose default norm is "BN".  Compute happens in the owning
    stack."""

    def __init__(self, dim, dim_res, norm="BN"):
        super().__init__()
        check_norm(norm, False)
        self.block = nn.Sequential(nn.ReLU(True), norm_layer(nn.Conv2d(dim, dim_res, 3, 1, 1), norm), nn.ReLU(True),
                                   norm_layer(nn.Conv2d(dim_res, dim, 1), norm))


class _TokensIn(torch.autograd.Function):
    """(B, C, T, H, W) -> token-major (B*T*H*W, C)."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = tuple(x.shape)
        B, C = x.shape[:2]
        R = x[0, 0].numel()
        return ew.to_channels_last(x.contiguous().view(B, C, R), C).view(B * R, C)

    @staticmethod
    def backward(ctx, g):
        B, C = ctx.shape[:2]
        R = g.shape[0] // B
        return ew.to_channels_first(g.contiguous().view(B, R, C), C).view(ctx.shape)


class _TokensOut(torch.autograd.Function):
    """token-major (B*R, C) -> (B, C, T, H, W)."""

    @staticmethod
    def forward(ctx, tok, B, C, T, H, W):
        return ew.to_channels_first(tok.contiguous().view(B, T * H * W, tok.shape[-1]), C).view(B, C, T, H, W)

    @staticmethod
    def backward(ctx, g):
        B, C = g.shape[:2]
        R = g[0, 0].numel()
        return ew.to_channels_last(g.contiguous().view(B, C, R), C).view(B * R, C), None, None, None, None, None

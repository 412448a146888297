"""Fused conv-stack executor: runs a chain of (transposed) convolutions with bias / ReLU / LeakyReLU / tanh / sigmoid /
residual epilogues on the implicit-GEMM engine, 2x2 average pools and nearest upsamples between them, and its hand-scheduled
backward.

Every activation is stored once, post-activation and channels-last.  ReLU backward is folded into
the epilogue of the kernel that produces the upstream gradient (mask = saved post-ReLU output) and
residual gradients are added in the same epilogue, so the backward chain is two or three engine
launches per layer (bwd-data, bwd-weight [+ bias column-sum where the weight-gradient kernel does not
produce it]) with no stand-alone elementwise pass.

Routing (round 2): the 3x3 and 4x4/stride-2 layers between 16x16 and 32x32 frames run on the
frame-resident kernels -- forward through `conv_fwd` (3x3) / `conv_fwd(wq=...)` (strided, parity classes),
transposed passes through `conv_bwd_data(wt=...)` (3x3, as a forward convolution over transposed weights) /
`conv_bwd_data(wph=...)` (stride 2, phase by phase), weight gradients inside `conv_bwd_weight`.  The extra
weight packs are made next to the forward one; every other geometry takes the implicit-GEMM engine.

Batch normalisation (Layer.norm, csrc/norm.hip): a normalised layer runs its conv with no bias, activation or residual
and keeps that pre-norm output; the statistics, finalize and apply kernels then write the layer's output (activation and
residual in the apply).  Its backward runs the BN backward (reduce + apply) between the incoming gradient and the conv's
weight and data gradients; the residual branch still receives the gradient at the add.  A no-grad forward whose norms
all use running statistics folds them into the conv weight and bias instead and runs the plain stack.

Resampling (Layer.kind "pool" / "up", csrc/resample.hip): parameter-less layers whose list entries in `params`, the weight packs
and the gradients are (None, None) / None, so layer indices (res_from, norms) count them.  Each is the other's backward -- pool
with scale 1 under an upsample, upsample with scale 0.25 under a pool -- and that launch applies the (Leaky)ReLU mask of the layer
in front, like the data-gradient epilogues of the convolutions.

Pixel shuffle (Layer.kind "shuffle", csrc/shuffle.hip): nn.PixelShuffle(2) with the activation behind it, parameter-less like the
resampling layers but with an `act` of its own -- ReLU, tanh and sigmoid are elementwise and commute with the permutation, so
outs[i] stays the post-activation output of layer i and the backward of that activation happens where it does for a convolution
(the head for tanh / sigmoid, the mask in the next layer's data-gradient epilogue for ReLU).  The convolution in front carries no
activation; the shuffle's own backward is the inverse permutation.
"""

import torch

from . import binding as L
from . import gemm as G
from . import ew
from . import norm as BN

class Layer:
    """One conv / ConvTranspose layer of a stack.

    kind: "conv" | "convT" | "pool" | "up" | "shuffle" ("pool" / "up": AvgPool2d(2) / Upsample(scale_factor=2); no parameters, no
    activation, no norm, cin == cout; see Layer.resample.  "shuffle": PixelShuffle(2); no parameters, no norm, cin == 4 cout, act
    "" | "relu" | "tanh" | "sigmoid"; see Layer.shuffle).  For convT the geometry is that of the equivalent forward conv whose
    backward-data IS this layer (Ci = out channels of the ConvTranspose, Co = its in channels).
    act: "" | "relu" | "leaky" (LeakyReLU(0.2)) | "tanh" | "sigmoid" (the last two on the last layer of a stack only).  res_from: index of an earlier
    output added before the activation (-1: none).  ci_real / co_real: channel counts of the torch-layout weight (pads excluded).
    norm: "" | "bn" | "syncbn" | "frozen": batch normalisation between the conv and the residual add / activation; the
    module that holds its tensors is handed to stack_forward per call (`norms`).
    """

    def __init__(self, kind, kernel, stride, pad, cin, cout, act="", res_from=-1, norm=""):
        self.kind, self.kernel, self.stride, self.pad = kind, kernel, stride, pad
        self.cin, self.cout, self.act, self.res_from = cin, cout, act, res_from
        self.norm = norm
        self.resamples = kind in ("pool", "up", "shuffle")

    @staticmethod
    def pad4(c):
        return (c + 3) // 4 * 4

    @classmethod
    def resample(cls, kind, channels):
        assert kind in ("pool", "up")
        return cls(kind, None, None, None, channels, channels)

    @classmethod
    def shuffle(cls, channels, act=""):
        """PixelShuffle(2) to `channels` channels, followed by `act`."""
        assert act in ("", "relu", "tanh", "sigmoid")
        return cls("shuffle", None, None, None, 4 * channels, channels, act=act)

    def resampled_shape(self, shape):
        """Channels-last output shape of a parameter-less layer."""
        N, T, H, W, Cp = shape
        if self.kind == "pool":
            return (N, T, H // 2, W // 2, Cp)
        return (N, T, 2 * H, 2 * W, Cp if self.kind == "up" else Layer.pad4(self.cout))


def _geom(layer, x_shape):
    """Geometry of the forward conv the engine sees, given the channels-last input shape."""
    N, T, H, W, _ = x_shape
    ci, co = Layer.pad4(layer.cin), Layer.pad4(layer.cout)
    if layer.kind == "conv":
        return G.conv_geom(N, T, H, W, ci, co, layer.kernel, layer.stride, layer.pad)
    # ConvTranspose: output extent = (in - 1) * s - 2p + k ; equivalent conv maps output -> input
    To, Ho, Wo = [(i - 1) * s - 2 * p + k for i, s, p, k in zip((T, H, W), layer.stride, layer.pad, layer.kernel)]
    g = G.conv_geom(N, To, Ho, Wo, co, ci, layer.kernel, layer.stride, layer.pad)
    assert (g.To, g.Ho, g.Wo) == (T, H, W), "ConvTranspose geometry mismatch"
    return g


def _padded_bias(layer, b):
    co = Layer.pad4(layer.cout)
    if b is None or b.numel() == co:
        return b
    return torch.cat([b, b.new_zeros(co - b.numel())])


def _act_flag(ly):
    """Epilogue flags of the layer's activation.  sigmoid(0) is not 0: its flag carries the number of pad channels, which the
    kernels then store as 0 like every other epilogue does by itself."""
    if ly.act == "sigmoid":
        return L.EPI_SIGMOID | L.epi_pad(Layer.pad4(ly.cout) - ly.cout)
    return {"": 0, "relu": L.EPI_RELU, "leaky": L.EPI_LEAKY, "tanh": L.EPI_TANH}[ly.act]


def _world():
    dist = torch.distributed
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _batch_stats(ly, nm):
    """The layer normalises with the statistics of the batch (nn.BatchNorm2d / NaiveSyncBatchNorm in train mode)."""
    return ly.norm in ("bn", "syncbn") and nm.training


def _running_affine(ly, nm):
    """(scale, shift, saved) of a layer that normalises with its running statistics (eval, FrozenBN)."""
    co = Layer.pad4(ly.cout)
    return BN.finalize(ly.cout, co, nm.weight, nm.bias, nm.running_mean, nm.running_var, eps=nm.eps, flags=L.BN_RUNNING)


def _normalise(ly, nm, y, res):
    """Statistics, finalize and apply of one normalised layer.  -> (out, (scale, saved, batch_stats, nranks))."""
    co = Layer.pad4(ly.cout)
    if _batch_stats(ly, nm):
        if nm.momentum is None:
            raise L.LvtError("BatchNorm momentum=None (cumulative average) is not implemented")
        st = BN.stats(y)
        nranks = _world() if ly.norm == "syncbn" else 1
        if nranks > 1:
            # one collective per layer: every rank fills its own slot of a zeroed (world, 2, Cp) buffer and the SUM gathers
            # them exactly (adding zeros rounds nothing), so the merge order is the same on every rank
            allst = torch.zeros(nranks, 2, co, dtype=torch.float32, device=y.device)
            allst[torch.distributed.get_rank()].copy_(st)
            torch.distributed.all_reduce(allst)
            st, flags = allst, L.BN_UPDATE
        else:
            flags = L.BN_UPDATE | L.BN_UNBIASED | L.BN_COUNT
        scale, shift, saved = BN.finalize(ly.cout, co, nm.weight, nm.bias, nm.running_mean, nm.running_var, stats=st,
                                          nranks=nranks, count=y.numel() // co, num_batches_tracked=nm.num_batches_tracked,
                                          momentum=nm.momentum, eps=nm.eps, flags=flags)
        batch = True
    else:
        scale, shift, saved = _running_affine(ly, nm)
        nranks, batch = 1, False
    out = BN.apply(y, scale, shift, res=res, act=_act_flag(ly))
    return out, (scale, saved, batch, nranks)


def stack_forward(layers, x, params, want_grad=True, norms=None):
    """x: (N,T,H,W,C) channels-last.  params: [(weight, bias)] in torch layout.  want_grad: a backward pass will follow
    (the transposed weight packs it needs are made here, next to the forward ones).  norms: per layer, the module holding
    its batch-normalisation tensors (None: no norm anywhere).
    Returns (outs, saved) where outs[i] is the post-activation output of layer i."""
    outs, geoms, packed = [], [], []
    norms = norms if norms is not None else [None] * len(layers)
    # eval fold: a forward without backward whose norms all use running statistics folds them into the conv weight and
    # bias (w' = w scale, b' = shift) and then runs exactly the kernels of the plain stack
    if not want_grad and all(nm is None or not _batch_stats(ly, nm) for ly, nm in zip(layers, norms)):
        todo = [i for i, nm in enumerate(norms) if nm is not None]
        if todo:
            params = list(params)
            folded = BN.fold([(params[i][0].detach(), layers[i].kind == "convT", norms[i], Layer.pad4(layers[i].cout))
                              for i in todo])          # one launch for the whole stack
            for i, wb in zip(todo, folded):
                params[i] = wb
        norms = [None] * len(layers)
    # every weight pack of the stack in ONE launch up front (24 ~5 us launches per VQ-VAE pass otherwise, each in front of the
    # layer that needs it): the geometries follow from the shapes alone
    pb = G.PackBatch()
    shape = tuple(x.shape)
    for i, (ly, (w, b)) in enumerate(zip(layers, params)):
        if ly.resamples:
            shape = ly.resampled_shape(shape)
            geoms.append(None)
            packed.append(None)
            continue
        g = _geom(ly, shape)
        wt = wph = wq = None
        if ly.kind == "conv":
            wp = pb.plain(g, w, ly.cin, ly.cout)
            if want_grad and i > 0 and G.bwd_data_by_phases(g):
                wph = pb.phases(g, w, ly.cin, ly.cout)          # for this layer's backward-data
            if G.fwd_by_parity(g):
                wq = pb.parity(g, w, ly.cin, ly.cout)           # this layer's forward (4x4 / stride 2)
            # backward-data of the 3x3 layers runs as a forward convolution over transposed weights (frame-resident kernel)
            if want_grad and G.bwd_data_as_conv(g):
                wt = pb.t(g, w, ly.cin, ly.cout)
            shape = (g.N, g.To, g.Ho, g.Wo, g.Co)
        else:
            wp = pb.plain(g, w, ly.cout, ly.cin)   # ConvTranspose weight is (in, out, k..) == conv (Co, Ci)
            if G.bwd_data_by_phases(g):
                wph = pb.phases(g, w, ly.cout, ly.cin)          # this layer's FORWARD is a transposed pass
            if want_grad and G.fwd_by_parity(g):
                wq = pb.parity(g, w, ly.cout, ly.cin)           # its backward-data is the strided convolution
            shape = (g.N, g.Ti, g.Hi, g.Wi, g.Ci)
        geoms.append(g)
        packed.append((wp, wt, wph, wq))
    pb.launch()
    cur = x
    pre, bn_saved = [None] * len(layers), [None] * len(layers)
    for i, (ly, (w, b)) in enumerate(zip(layers, params)):
        if ly.resamples:
            if ly.kind == "shuffle":
                cur = ew.pixel_shuffle2(cur, ly.cout, ly.act)
            else:
                cur = ew.pool2x2(cur) if ly.kind == "pool" else ew.upsample2x2(cur)
            outs.append(cur)
            continue
        g, (wp, wt, wph, wq) = geoms[i], packed[i]
        nm = norms[i]
        seen = (g.N, g.Ti, g.Hi, g.Wi) if ly.kind == "conv" else (g.N, g.To, g.Ho, g.Wo)
        assert seen == tuple(cur.shape[:4]), "geometry of the pre-pass does not match the activation"
        res = outs[ly.res_from] if ly.res_from >= 0 else None
        if nm is not None:
            # the conv alone; bias, residual and activation belong to the normalised output
            if ly.kind == "conv":
                y = G.conv_fwd(g, cur, wp, wq=wq)
            else:
                y = G.conv_bwd_data(g, cur, wp, wph=wph)
            pre[i] = y
            y, bn_saved[i] = _normalise(ly, nm, y, res)
            outs.append(y)
            cur = y
            continue
        bias = _padded_bias(ly, b)
        if ly.kind == "conv":
            y = G.conv_fwd(g, cur, wp, bias=bias, res=res, flags=_act_flag(ly), wq=wq)
        elif (ly.cout <= 3 and ly.kernel == (1, 4, 4) and ly.stride == (1, 2, 2) and ly.pad == (0, 1, 1)
              and ly.cin % 16 == 0 and res is None and ly.act in ("", "tanh", "sigmoid")):
            y = G.convT4_fwd(cur, w, b, _act_flag(ly) & (L.EPI_TANH | L.EPI_SIGMOID))          # image-side layer: dedicated kernel
        else:
            y = G.conv_bwd_data(g, cur, wp, bias=bias, res=res, flags=_act_flag(ly), wph=wph)
        outs.append(y)
        cur = y
    return outs, (geoms, packed, norms, pre, bn_saved)


def _bn_backward(ly, nm, gp, y, bn_saved):
    """BN backward of one layer: gp is the gradient at the normalised output (mask and residual already folded in).
    -> (gradient at the conv output, (dgamma, dbeta) or None)."""
    scale, saved, batch, nranks = bn_saved
    co = Layer.pad4(ly.cout)
    if ly.norm == "frozen":
        return BN.bwd_apply(gp, None, scale, train=False), None
    sums = BN.bwd_reduce(gp, y, saved)
    dg = (sums[1, :ly.cout].clone(), sums[0, :ly.cout].clone())
    if not batch:
        return BN.bwd_apply(gp, None, scale, train=False), dg
    if nranks > 1:
        # the statistics' gradients summed over the ranks (the reference's AllReduce.backward): one collective per layer
        sums = sums.clone()
        torch.distributed.all_reduce(sums)
    return BN.bwd_apply(gp, y, scale, saved, sums, n=nranks * (y.numel() // co), train=True), dg


def stack_backward(layers, x, outs, saved, grad_out, need_input_grad=False):
    """grad_out: dL/d(outs[-1]) (post-activation).  Returns (grad_x or None, [(dw, db)], [(dgamma, dbeta)]); db is None for
    a normalised layer, (dw, db) is (None, None) for a pool / upsample / shuffle layer, and the last list holds the layers with trainable
    norms in stack order."""
    geoms, packed, norms, pre, bn_saved = saved
    n = len(layers)
    # g_pre of the last layer
    last = layers[-1]
    if last.act == "tanh":
        gpre = ew.tanh_bwd(grad_out, outs[-1])
    elif last.act == "sigmoid":
        gpre = ew.sigmoid_bwd(grad_out, outs[-1])
    elif last.act in ("relu", "leaky"):
        raise L.LvtError("a ReLU-terminated stack is not used by the reference architectures")
    else:
        gpre = grad_out
    # residual consumers: res_grad[j] = g_pre of the layer that used outs[j] as its residual
    res_user = {ly.res_from: i for i, ly in enumerate(layers) if ly.res_from >= 0}
    gpres = [None] * n
    gpres[n - 1] = gpre
    grads = [None] * n
    norm_grads = [None] * n
    gx = None
    for i in range(n - 1, -1, -1):
        ly = layers[i]
        if ly.resamples:
            # the dual kernel, with the activation backward of the layer in front folded in
            grads[i] = (None, None)
            if i == 0 and not need_input_grad:
                break
            prev = layers[i - 1] if i > 0 else None
            if ly.kind == "shuffle":
                # the inverse permutation; this layer's own activation was undone by the head or by the mask of the layer behind
                if (i - 1) in res_user or (prev is not None and prev.act):
                    raise L.LvtError("a pixel shuffle must follow a convolution without activation that is no residual source")
                gin = ew.pixel_unshuffle2(gpres[i], ly.cout)
                if i > 0:
                    gpres[i - 1] = gin
                else:
                    gx = gin
                continue
            if (i - 1) in res_user or (prev is not None and prev.act in ("tanh", "sigmoid")):
                raise L.LvtError("a pool / upsample layer follows conv + (Leaky)ReLU layers only")
            mask = outs[i - 1] if (prev is not None and prev.act in ("relu", "leaky")) else None
            leaky = prev is not None and prev.act == "leaky"
            if ly.kind == "pool":
                gin = ew.upsample2x2(gpres[i], 0.25, mask=mask, leaky=leaky)
            else:
                gin = ew.pool2x2(gpres[i], 1.0, mask=mask, leaky=leaky)
            if i > 0:
                gpres[i - 1] = gin
            else:
                gx = gin
            continue
        g, (wp, wt, wph, wq) = geoms[i], packed[i]
        inp = outs[i - 1] if i > 0 else x
        gp = gpres[i]
        if norms[i] is not None:
            gp, norm_grads[i] = _bn_backward(ly, norms[i], gp, pre[i], bn_saved[i])
        # parameter gradients
        co = Layer.pad4(ly.cout)
        db = None
        if norms[i] is not None:
            # a normalised conv has no bias
            if ly.kind == "conv":
                dw = G.conv_bwd_weight(g, inp, gp, ly.cin, ly.cout)
            else:
                dw = G.conv_bwd_weight(g, gp, inp, ly.cout, ly.cin)
        elif ly.kind == "conv":
            dw, db = G.conv_bwd_weight(g, inp, gp, ly.cin, ly.cout, want_bias=True)     # db rides on the dy stream
        else:
            # transposed layer: the same call with the operands swapped; its bias gradient is the column sum of gp, which the
            # stride-2 frame-resident kernel adds up from the patches it stages
            dw, db = G.conv_bwd_weight(g, gp, inp, ly.cout, ly.cin, want_bias=True, bias_of_x=True)
        if norms[i] is None and db is None:
            db = G.colsum(gp, gp.numel() // co, co)[:ly.cout]
        grads[i] = (dw, db)      # dw is (Co, Ci, Kt, Kh, Kw); callers view it as the parameter shape
        # gradient w.r.t. the layer input == g_pre of layer i-1 (mask / residual folded in)
        if i == 0 and not need_input_grad:
            break
        prev = layers[i - 1] if i > 0 else None
        res = gpres[res_user[i - 1]] if (i - 1) in res_user else None
        mask = outs[i - 1] if (prev is not None and prev.act in ("relu", "leaky")) else None
        lk = L.EPI_LEAKY_MASK if (prev is not None and prev.act == "leaky") else 0
        if prev is not None and prev.act in ("tanh", "sigmoid"):
            raise L.LvtError("%s is only supported on the last layer of a stack" % prev.act)
        if ly.kind == "conv":
            gin = G.conv_bwd_data(g, gp, wp, res=res, mask=mask, flags=lk, wt=wt, wph=wph)
        else:
            gin = G.conv_fwd(g, gp, wp, res=res, mask=mask, flags=lk, wq=wq)
        if i > 0:
            gpres[i - 1] = gin
        else:
            gx = gin
    return gx, grads, [d for d in norm_grads if d is not None]

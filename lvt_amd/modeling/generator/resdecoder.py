"""Residual conv decoders (reference: vidgen/modeling/generator/resdecoder.py:25-129).

    ResDecoder         Conv(k3 p1), n x ResBlock, ReLU, ConvT(k4 s2 p1)+ReLU, ConvT(k4 s2 p1) [, tanh | sigmoid]
    ResShuffleDecoder  Conv(k3 p1), n x ResBlock, ReLU, Conv(k3 p1)+PixelShuffle(2)+ReLU, Conv(k3 p1)+PixelShuffle(2) [, tanh | sigmoid]

ConvTranspose layers run as the backward-data form of the implicit-GEMM engine, decomposed by
output stride phase so that no matrix-core work is spent on structurally-zero taps.  The sub-pixel decoder's 3x3 convolutions are
the frame-resident kernels of the trunk at 16x16 and 32x32; each PixelShuffle is one streaming launch that also applies the
activation behind it (hip/convnet.py, Layer.kind "shuffle").  The two classes share everything but the upscaling tail.
"""
from torch import nn

from ...hip.convnet import Layer
from .. import convstack
from .build import GENERATOR_REGISTRY
from .generator import Generator


class _ResTrunkDecoder(Generator):
    """Trunk, output activation, plan and forward of both decoders; `_upscale` is the tail between them."""

    @classmethod
    def from_config(cls, cfg, **kwargs):
        g = cfg.MODEL.GENERATOR
        return cls(in_channels=g.IN_CHANNELS, nf=g.NF, res_channels=g.RES_CHANNELS, out_channels=g.OUT_CHANNELS,
                   norm=g.NORM, use_spectral_norm=g.SPECTRAL, n_layers=g.N_LAYERS,
                   out_activation=kwargs.get("out_activation", g.OUT_ACTIVATION), stride=kwargs.get("stride", 4))

    def __init__(self, in_channels, nf, res_channels, out_channels, norm, use_spectral_norm, n_layers,
                 out_activation, stride):
        super().__init__()
        convstack.check_norm(norm, use_spectral_norm)
        norm = norm or ""
        nl = convstack.norm_layer
        mods = [nl(nn.Conv2d(in_channels, nf, 3, 1, 1), norm)]
        mods += [convstack.ResBlock(nf, res_channels, norm) for _ in range(n_layers)]
        mods.append(nn.ReLU(True))
        mods += self._upscale(nf, out_channels, norm, stride)
        out_act = convstack.out_activation_module(out_activation)
        if out_act is not None:
            mods.append(out_act)
        self.layers = nn.Sequential(*mods)
        self.in_channels, self.out_channels = in_channels, out_channels
        self._plan = self._build_plan()

    def _build_plan(self):
        mods = list(self.layers)
        plan, owners, norms = [], [], []
        for i, m in enumerate(mods):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            act = convstack.act_after(nxt)
            if convstack.is_conv(m, nn.Conv2d) or convstack.is_conv(m, nn.ConvTranspose2d):
                m, nm, kind = convstack.split_norm(m)
                k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
                plan.append(Layer("convT" if isinstance(m, nn.ConvTranspose2d) else "conv", (1, k, k), (1, s, s), (0, p, p),
                                  m.in_channels, m.out_channels, act=act, norm=kind))
                owners.append(m)
                norms.append(nm)
            elif isinstance(m, convstack.ResBlock):
                (c3, n3, k3), (c1, n1, k1) = convstack.split_norm(m.block[1]), convstack.split_norm(m.block[3])
                src = len(plan) - 1
                plan.append(Layer("conv", (1, 3, 3), (1, 1, 1), (0, 1, 1), c3.in_channels, c3.out_channels, act="relu",
                                  norm=k3))
                owners.append(c3)
                norms.append(n3)
                plan.append(Layer("conv", (1, 1, 1), (1, 1, 1), (0, 0, 0), c1.in_channels, c1.out_channels, act=act,
                                  res_from=src, norm=k1))
                owners.append(c1)
                norms.append(n1)
            elif isinstance(m, nn.PixelShuffle):
                if m.upscale_factor != 2 or not plan or plan[-1].cout % 4:
                    raise NotImplementedError("only PixelShuffle(2) behind a convolution to 4 C channels: %r" % (m,))
                plan.append(Layer.shuffle(plan[-1].cout // 4, act=act))
                owners.append(None)
                norms.append(None)
        self._owners = owners
        self._norms = norms if any(n is not None for n in norms) else None      # NORM "": the plain stack, as before
        return plan

    def forward_cl(self, z_cl):
        """(N,1,h,w,Cin) channels-last -> (N,1,4h,4w,Cout_pad4)."""
        return convstack.run_stack(z_cl, self._plan, convstack.plan_params(self._owners), self._norms)

    def forward(self, z):
        y = self.forward_cl(convstack._LayoutIn.apply(z))
        return convstack._LayoutOut.apply(y, self.out_channels)


@GENERATOR_REGISTRY.register()
class ResDecoder(_ResTrunkDecoder):
    @staticmethod
    def _upscale(nf, out_channels, norm, stride):
        nl = convstack.norm_layer
        if stride == 4:
            # the last ConvTranspose is never normalised (resdecoder.py:55-59)
            return [nl(nn.ConvTranspose2d(nf, nf // 2, 4, 2, 1), norm), nn.ReLU(True),
                    nn.ConvTranspose2d(nf // 2, out_channels, 4, 2, 1)]
        if stride == 2:
            # ... except at stride 2, where it is the only one and the reference normalises it (resdecoder.py:60-63)
            return [nl(nn.ConvTranspose2d(nf, out_channels, 4, 2, 1), norm)]
        raise ValueError


@GENERATOR_REGISTRY.register()
class ResShuffleDecoder(_ResTrunkDecoder):
    """Sub-pixel variant (resdecoder.py:78-129): each ConvTranspose2d(4, 2, 1) becomes Conv2d(3, 1, 1) to four times the channels
    and PixelShuffle(2).  Which convolutions are normalised follows ResDecoder's rule."""

    @staticmethod
    def _upscale(nf, out_channels, norm, stride):
        nl = convstack.norm_layer
        if stride == 4:
            return [nl(nn.Conv2d(nf, nf // 2 * 4, 3, 1, 1), norm), nn.PixelShuffle(2), nn.ReLU(True),
                    nn.Conv2d(nf // 2, out_channels * 4, 3, 1, 1), nn.PixelShuffle(2)]
        if stride == 2:
            return [nl(nn.Conv2d(nf, out_channels * 4, 3, 1, 1), norm), nn.PixelShuffle(2)]
        raise ValueError

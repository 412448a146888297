"""Residual conv encoder (reference: vidgen/modeling/encoder/resencoder.py:25-76).

Same constructor / `from_config` / state_dict keys (`layers.N.weight`, `layers.N.block.M.weight`);
the forward pass is one fused chain of implicit-GEMM kernels on channels-last activations:

    stride 4:  Conv(k4 s2 p1)+ReLU, Conv(k4 s2 p1)+ReLU, Conv(k3 p1), n x ResBlock [, sigmoid | tanh]

The reference's ResBlock starts with an in-place ReLU, so the block input itself is rectified and
the skip adds relu(x).  That ReLU is therefore folded into the epilogue of the layer
that PRODUCES x, which is what makes the whole stack a chain of conv+epilogue kernels.
"""
from torch import nn

from ...hip.convnet import Layer
from .. import convstack
from .build import ENCODER_REGISTRY
from .encoder import Encoder


@ENCODER_REGISTRY.register()
class ResEncoder(Encoder):
    @classmethod
    def from_config(cls, cfg, **kwargs):
        e = cfg.MODEL.ENCODER
        return cls(in_channels=kwargs.get("in_channels", e.IN_CHANNELS), nf=e.NF, res_channels=e.RES_CHANNELS,
                   norm=e.NORM, use_spectral_norm=e.SPECTRAL, n_layers=e.N_LAYERS,
                   out_activation=e.OUT_ACTIVATION, stride=kwargs.get("stride", 4))

    def __init__(self, in_channels, nf, res_channels, norm, use_spectral_norm, n_layers, out_activation, stride):
        super().__init__()
        convstack.check_norm(norm, use_spectral_norm)
        if out_activation == "relu":
            # the reference's encoder also knows "relu"; a ReLU-terminated stack has no backward here (hip/convnet.py)
            raise NotImplementedError("ResEncoder out_activation 'relu' is not implemented")
        out_act = convstack.out_activation_module(out_activation)
        norm = norm or ""
        nl = convstack.norm_layer
        if stride == 4:
            mods = [nl(nn.Conv2d(in_channels, nf // 2, 4, 2, 1), norm), nn.ReLU(True), nl(nn.Conv2d(nf // 2, nf, 4, 2, 1), norm),
                    nn.ReLU(True), nl(nn.Conv2d(nf, nf, 3, 1, 1), norm)]
        elif stride == 2:
            mods = [nl(nn.Conv2d(in_channels, nf // 2, 4, 2, 1), norm), nn.ReLU(True), nl(nn.Conv2d(nf // 2, nf, 3, 1, 1), norm)]
        else:
            raise ValueError
        mods += [convstack.ResBlock(nf, res_channels, norm) for _ in range(n_layers)]
        if out_act is not None:
            mods.append(out_act)
        self.layers = nn.Sequential(*mods)
        self.in_channels, self.out_channels = in_channels, nf
        self._plan = self._build_plan()

    def _build_plan(self):
        """Translate the module list into fused engine layers + the (weight, bias) modules they use."""
        mods = list(self.layers)
        plan, owners, norms = [], [], []
        for i, m in enumerate(mods):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            # this output is rectified if an explicit ReLU or a ResBlock (in-place ReLU) follows, bounded if the output
            # activation does
            act = convstack.act_after(nxt)
            if convstack.is_conv(m, nn.Conv2d):
                m, nm, kind = convstack.split_norm(m)
                k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
                plan.append(Layer("conv", (1, k, k), (1, s, s), (0, p, p), m.in_channels, m.out_channels,
                                  act=act, norm=kind))
                owners.append(m)
                norms.append(nm)
            elif isinstance(m, convstack.ResBlock):
                (c3, n3, k3), (c1, n1, k1) = convstack.split_norm(m.block[1]), convstack.split_norm(m.block[3])
                src = len(plan) - 1          # output index of the (rectified) block input
                plan.append(Layer("conv", (1, 3, 3), (1, 1, 1), (0, 1, 1), c3.in_channels, c3.out_channels, act="relu",
                                  norm=k3))
                owners.append(c3)
                norms.append(n3)
                # the residual is added after the second norm: relu(x) + BN(conv1x1(relu(BN(conv3x3(relu(x))))))
                plan.append(Layer("conv", (1, 1, 1), (1, 1, 1), (0, 0, 0), c1.in_channels, c1.out_channels,
                                  act=act, res_from=src, norm=k1))
                owners.append(c1)
                norms.append(n1)
        self._owners = owners
        self._norms = norms if any(n is not None for n in norms) else None      # NORM "": the plain stack, as before
        return plan

    def forward_cl(self, x_cl):
        """(N,1,H,W,Cin_pad4) channels-last -> (N,1,H/4,W/4,nf)."""
        return convstack.run_stack(x_cl, self._plan, [(m.weight, m.bias) for m in self._owners], self._norms)

    def forward(self, x):
        """(N,C,H,W) -> (N,nf,H/4,W/4), the reference's layout contract."""
        y = self.forward_cl(convstack._LayoutIn.apply(x))
        return convstack._LayoutOut.apply(y, self.out_channels)

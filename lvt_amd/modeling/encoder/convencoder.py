"""Plain conv encoder (reference: vidgen/modeling/encoder/convencoder.py:11-68).

Same constructor / `from_config` / module tree / state_dict keys (`layers.N.weight`, or `layers.N.0.weight` and `layers.N.1.*`
when normalised); the forward pass is one chain of conv + LeakyReLU(0.2) epilogue launches with a 2x2 average pool between the
scales:

    Conv(k3 p1)+Leaky, n x [Conv(k3 p1)+Leaky, Conv(k3 p1)+Leaky, AvgPool(2)], Conv(k3 p1)+Leaky, Conv(k3 p1) [, sigmoid | tanh]

Every convolution is normalised when NORM is set, the last one included.
"""
from torch import nn

from ...hip.convnet import Layer
from .. import convstack
from .build import ENCODER_REGISTRY
from .encoder import Encoder


@ENCODER_REGISTRY.register()
class ConvEncoder(Encoder):
    @classmethod
    def from_config(cls, cfg, **kwargs):
        e = cfg.MODEL.ENCODER
        return cls(in_channels=e.IN_CHANNELS, nf=e.NF, out_channels=e.OUT_CHANNELS, norm=e.NORM,
                   use_spectral_norm=e.SPECTRAL, n_layers=e.N_LAYERS, out_activation=e.OUT_ACTIVATION)

    def __init__(self, in_channels, nf, out_channels, norm, use_spectral_norm, n_layers, out_activation):
        super().__init__()
        convstack.check_norm(norm, use_spectral_norm)
        out_act = convstack.out_activation_module(out_activation)      # "", sigmoid, tanh; anything else is a ValueError
        norm = norm or ""

        def conv(ci, co):
            return convstack.norm_layer(nn.Conv2d(ci, co, 3, stride=1, padding=1), norm)

        mods = [conv(in_channels, nf), nn.LeakyReLU(0.2, True)]
        kp = nf
        for i in range(n_layers):
            k = nf << i
            mods += [conv(kp, k), nn.LeakyReLU(0.2, True), conv(k, k), nn.LeakyReLU(0.2, True), nn.AvgPool2d(2)]
            kp = k
        k = nf << n_layers
        mods += [conv(kp, k), nn.LeakyReLU(0.2, True), conv(k, out_channels)]
        if out_act is not None:
            mods.append(out_act)
        self.layers = nn.Sequential(*mods)
        self.in_channels, self.out_channels = in_channels, out_channels
        self._plan, self._owners, self._norms = convstack.plain_plan(self.layers)

    def forward_cl(self, x_cl):
        """(N,1,H,W,Cin_pad4) channels-last -> (N,1,H >> n_layers,W >> n_layers,Cout_pad4)."""
        return convstack.run_stack(x_cl, self._plan, convstack.plan_params(self._owners), self._norms)

    def forward(self, x):
        """(N,C,H,W) -> (N,out_channels,H >> n_layers,W >> n_layers), the reference's layout contract."""
        y = self.forward_cl(convstack._LayoutIn.apply(x))
        return convstack._LayoutOut.apply(y, self.out_channels)

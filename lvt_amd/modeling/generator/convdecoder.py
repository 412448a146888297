"""Plain conv decoder (reference: vidgen/modeling/generator/convdecoder.py:10-57).

    n x [Conv(k3 p1)+Leaky, Conv(k3 p1)+Leaky, Upsample(2)], Conv(k3 p1), Conv(k3 p1) [, tanh | sigmoid]

Same constructor / `from_config` / module tree / state_dict keys.  The last two convolutions are never normalised, keep
their bias and have no activation between them; the second of them reads as many channels as the first (the reference
builds both from the width of the last scale), so the pair only composes when that width equals NF -- always true with
N_LAYERS >= 1, and with N_LAYERS 0 exactly when IN_CHANNELS == NF.
"""
from torch import nn

from .. import convstack
from .build import GENERATOR_REGISTRY
from .generator import Generator


@GENERATOR_REGISTRY.register()
class ConvDecoder(Generator):
    @classmethod
    def from_config(cls, cfg, **kwargs):
        g = cfg.MODEL.GENERATOR
        return cls(in_channels=g.IN_CHANNELS, nf=g.NF, out_channels=g.OUT_CHANNELS, norm=g.NORM,
                   use_spectral_norm=g.SPECTRAL, n_layers=g.N_LAYERS, out_activation=g.OUT_ACTIVATION)

    def __init__(self, in_channels, nf, out_channels, norm, use_spectral_norm, n_layers, out_activation):
        super().__init__()
        convstack.check_norm(norm, use_spectral_norm)
        out_act = convstack.out_activation_module(out_activation)
        norm = norm or ""

        def conv(ci, co, nm):
            return convstack.norm_layer(nn.Conv2d(ci, co, 3, stride=1, padding=1), nm)

        mods = []
        kp = in_channels
        for scale in range(n_layers - 1, -1, -1):
            k = nf << scale
            mods += [conv(kp, k, norm), nn.LeakyReLU(0.2, True), conv(k, k, norm), nn.LeakyReLU(0.2, True),
                     nn.Upsample(scale_factor=2)]
            kp = k
        if kp != nf:
            # the reference builds this module and fails in its first forward (a conv to nf channels feeds one that reads kp)
            raise ValueError("ConvDecoder: the last convolution reads %d channels but the one in front writes NF = %d "
                             "(N_LAYERS 0 needs IN_CHANNELS == NF)" % (kp, nf))
        mods += [conv(kp, nf, ""), conv(kp, out_channels, "")]
        if out_act is not None:
            mods.append(out_act)
        self.layers = nn.Sequential(*mods)
        self.in_channels, self.out_channels = in_channels, out_channels
        self._plan, self._owners, self._norms = convstack.plain_plan(self.layers)

    def forward_cl(self, z_cl):
        """(N,1,h,w,Cin) channels-last -> (N,1,h << n_layers,w << n_layers,Cout_pad4)."""
        return convstack.run_stack(z_cl, self._plan, convstack.plan_params(self._owners), self._norms)

    def forward(self, z):
        y = self.forward_cl(convstack._LayoutIn.apply(z))
        return convstack._LayoutOut.apply(y, self.out_channels)

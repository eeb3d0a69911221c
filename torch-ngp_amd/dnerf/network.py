"""D-NeRF network (reference dnerf/network.py:10-270): a deformation MLP in
front of the static field. forward(x, d, t): deform = deform_net([enc(x),
enc(t)]); the hash grid is sampled at x + deform (with its input gradient, so
the deformation trains through the grid); sigma_net reads [grid, enc(x),
enc(t)], color_net [sh(d), geo_feat]. Every layer is nn.Linear(bias=False)
under the reference's module names, so state_dict() has its keys and shapes.

[enc(x), enc(t)] is one launch (ngp_dnerf_encode, csrc/dnerf.hip) instead of
two encoder launches, a repeat and a cat, written in the autocast dtype; the
same tensor is the deformation network's input and the tail of the sigma
network's. encoder_deform / encoder_time stay as (parameter-free) modules for
get_params' groups and their output widths. Not included: the background
model, a fused deformation MLP."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from activation import trunc_exp
from encoding import get_encoder

from . import backend
from .renderer import NeRFRenderer


def _mlp(in_dim, hidden, out_dim, layers):
    return nn.ModuleList([nn.Linear(in_dim if l == 0 else hidden, out_dim if l == layers - 1 else hidden, bias=False)
                          for l in range(layers)])


def _run(net, h):
    for l, layer in enumerate(net):
        h = layer(h)
        if l != len(net) - 1:
            h = F.relu(h, inplace=True)
    return h


class NeRFNetwork(NeRFRenderer):
    def __init__(self, encoding="tiledgrid", encoding_dir="sphere_harmonics", encoding_time="frequency",
                 encoding_deform="frequency", num_layers=2, hidden_dim=64, geo_feat_dim=15, num_layers_color=3,
                 hidden_dim_color=64, num_layers_deform=5, hidden_dim_deform=128, bound=1, cuda_ray=True, **kwargs):
        super().__init__(bound, cuda_ray, **kwargs)
        if encoding_time != "frequency" or encoding_deform != "frequency":
            raise NotImplementedError("dnerf: the time and deformation encodings are the frequency ones "
                                      "(ngp_dnerf_encode: 10 and 6 octaves)")
        # deformation network
        self.num_layers_deform = num_layers_deform
        self.hidden_dim_deform = hidden_dim_deform
        self.encoder_deform, self.in_dim_deform = get_encoder(encoding_deform, multires=10)
        self.encoder_time, self.in_dim_time = get_encoder(encoding_time, input_dim=1, multires=6)
        assert self.in_dim_deform + self.in_dim_time == backend.ENCODE_COLS
        self.deform_net = _mlp(self.in_dim_deform + self.in_dim_time, hidden_dim_deform, 3, num_layers_deform)
        # sigma network
        self.num_layers = num_layers
        self.hidden_dim = hidden_dim
        self.geo_feat_dim = geo_feat_dim
        self.encoder, self.in_dim = get_encoder(encoding, desired_resolution=2048 * bound)
        self.sigma_net = _mlp(self.in_dim + self.in_dim_time + self.in_dim_deform, hidden_dim, 1 + geo_feat_dim,
                              num_layers)
        # colour network
        self.num_layers_color = num_layers_color
        self.hidden_dim_color = hidden_dim_color
        self.encoder_dir, self.in_dim_dir = get_encoder(encoding_dir)
        self.color_net = _mlp(self.in_dim_dir + geo_feat_dim, hidden_dim_color, 3, num_layers_color)
        self.bg_net = None

    def encode_xt(self, x, t):
        """[enc(x), enc(t)] [N, 76] in the autocast dtype; t [1, 1] or [N, 1]. Neither input is learnable."""
        dtype = torch.get_autocast_dtype("cuda") if torch.is_autocast_enabled() else torch.float32
        if dtype not in (torch.float16, torch.float32):
            dtype = torch.float32
        return backend.encode(x.detach().float().contiguous(), t.detach().float().contiguous(), dtype)

    def _density(self, x, t):
        enc = self.encode_xt(x, t)
        deform = _run(self.deform_net, enc)
        h = self.encoder(x + deform, bound=self.bound)
        h = _run(self.sigma_net, torch.cat([h, enc.to(h.dtype)], dim=1))
        return trunc_exp(h[..., 0]), h[..., 1:], deform

    def _color(self, d, geo_feat):
        d = self.encoder_dir(d)
        return torch.sigmoid(_run(self.color_net, torch.cat([d, geo_feat.to(d.dtype)], dim=-1)))

    def forward(self, x, d, t):
        """x [N, 3] in [-bound, bound], d [N, 3] unit, t [1, 1] or [N, 1] in [0, 1]
        -> sigma [N], rgbs [N, 3], deform [N, 3]."""
        sigma, geo_feat, deform = self._density(x, t)
        return sigma, self._color(d, geo_feat), deform

    def density(self, x, t):
        sigma, geo_feat, deform = self._density(x, t)
        return {"sigma": sigma, "geo_feat": geo_feat, "deform": deform}

    def color(self, x, d, mask=None, geo_feat=None, **kwargs):
        """Masked colour query (:223-252): rows outside the mask are zero."""
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            d, geo_feat = d[mask], geo_feat[mask]
        h = self._color(d, geo_feat)
        if mask is not None:
            rgbs[mask] = h.to(rgbs.dtype)
            return rgbs
        return h

    def get_params(self, lr, lr_net):
        return [
            {"params": self.encoder.parameters(), "lr": lr},
            {"params": self.sigma_net.parameters(), "lr": lr_net},
            {"params": self.encoder_dir.parameters(), "lr": lr},
            {"params": self.color_net.parameters(), "lr": lr_net},
            {"params": self.encoder_deform.parameters(), "lr": lr},
            {"params": self.encoder_time.parameters(), "lr": lr},
            {"params": self.deform_net.parameters(), "lr": lr_net},
        ]

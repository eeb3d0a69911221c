"""SDFNetwork (the reference's sdf/netowrk_ff.py): get_encoder followed by a
fully-fused MLP with one output."""
import torch.nn as nn

from encoding import get_encoder
from ffmlp import FFMLP


class SDFNetwork(nn.Module):
    def __init__(self, encoding="hashgrid", num_layers=3, hidden_dim=64, clip_sdf=None, skips=(), **encoder_kwargs):
        """encoder_kwargs go to get_encoder (e.g. log2_hashmap_size for a small table)."""
        super().__init__()
        self.num_layers = num_layers
        self.skips = list(skips)
        self.hidden_dim = hidden_dim
        self.clip_sdf = clip_sdf
        assert self.skips == [], "FFMLP does not support concatenating inside, please use skips=[]."
        self.encoder, self.in_dim = get_encoder(encoding, **encoder_kwargs)
        self.backbone = FFMLP(input_dim=self.in_dim, output_dim=1, hidden_dim=self.hidden_dim,
                              num_layers=self.num_layers)

    def forward(self, x):
        # x: [B, 3] in [-1, 1] -> [B, 1]
        h = self.backbone(self.encoder(x))
        if self.clip_sdf is not None:
            h = h.clamp(-self.clip_sdf, self.clip_sdf)
        return h

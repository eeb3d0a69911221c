"""TensoRF's NeRFNetwork (the reference's tensoRF/network.py) with the
vector-matrix decomposition sampled by csrc/tensorf.hip (tensoRF/vm.py).

Density: trunc_exp of the sum over the density set. Colour: the colour set's
products -> basis_mat (Linear, no bias) -> frequency encoding (multires 2) of
the 27 features and of the direction -> a 3-layer, 128-wide, bias-free ReLU
MLP -> sigmoid. The planes and lines are kept [H, W, R] and [D, R];
state_dict() and load_state_dict() speak the reference's [1, R, H, W] and
[1, R, D, 1], and load_state_dict() takes a checkpoint of any resolution.

Not included: --cp (network_cp) and CCNeRF; the background
model (bg_radius > 0 raises); patch sampling / LPIPS and CLIP; the GUI;
hipGraph capture; data-parallel training; device-written test frames and
video (the frame renderer is bound to the fused network)."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from activation import trunc_exp
from encoding import get_encoder
from nerf.renderer import NeRFRenderer

from .vm import (MAT_IDS, VEC_IDS, line_from_ref, line_to_ref, plane_from_ref, plane_to_ref, vm_sample)

_SETS = ("sigma_mat", "sigma_vec", "color_mat", "color_vec")


def morton3D_invert(indices):
    """Morton codes (x | y << 1 | z << 2 interleaved, 10 bits per axis) ->
    [n, 3] integer coordinates, in torch on the codes' device."""
    def compact(v):
        v = v & 0x09249249
        v = (v ^ (v >> 2)) & 0x030C30C3
        v = (v ^ (v >> 4)) & 0x0300F00F
        v = (v ^ (v >> 8)) & 0x030000FF
        v = (v ^ (v >> 16)) & 0x000003FF
        return v
    v = indices.reshape(-1).long()
    return torch.stack((compact(v), compact(v >> 1), compact(v >> 2)), -1)


def upsample_resolution(aabb, n_voxels):
    """The resolution of a model of about n_voxels cubic voxels inside aabb
    (lo, hi): the voxel edge is the cube root of the box volume over n_voxels,
    the resolution the extent over it, truncated (tensoRF/utils.py:119-122,
    float32 numpy as there)."""
    import numpy as np
    aabb = np.asarray(aabb, dtype=np.float32)
    extent = aabb[3:] - aabb[:3]
    vox_size = np.cbrt(np.prod(extent) / n_voxels)
    return (extent / vox_size).astype(np.int32).tolist()


def upsample_schedule(resolution0, resolution1, n_steps):
    """The target resolutions of the n_steps upsamplings: log-spaced between
    resolution0 and resolution1, the first left out (main_tensoRF.py:132)."""
    import numpy as np
    r = np.round(np.exp(np.linspace(np.log(resolution0), np.log(resolution1), n_steps + 1)))
    return r.astype(np.int32).tolist()[1:]


class NeRFNetwork(NeRFRenderer):
    def __init__(self, resolution=(128, 128, 128), sigma_rank=(16, 16, 16), color_rank=(48, 48, 48),
                 color_feat_dim=27, num_layers=3, hidden_dim=128, bound=1, **kwargs):
        super().__init__(bound, **kwargs)
        if self.bg_radius > 0:
            raise NotImplementedError("tensoRF: the background model (bg_radius > 0) is not included")
        self.resolution = [int(r) for r in resolution]
        self.sigma_rank, self.color_rank = list(sigma_rank), list(color_rank)
        self.color_feat_dim = color_feat_dim
        self.mat_ids, self.vec_ids = [list(m) for m in MAT_IDS], list(VEC_IDS)
        self.sigma_mat, self.sigma_vec = self._init_set(self.sigma_rank)
        self.color_mat, self.color_vec = self._init_set(self.color_rank)
        self.basis_mat = nn.Linear(sum(self.color_rank), color_feat_dim, bias=False)
        self.num_layers, self.hidden_dim = num_layers, hidden_dim
        self.encoder, enc_dim = get_encoder("frequency", input_dim=color_feat_dim, multires=2)
        self.encoder_dir, enc_dim_dir = get_encoder("frequency", input_dim=3, multires=2)
        self.in_dim = enc_dim + enc_dim_dir
        self.color_net = nn.ModuleList(
            nn.Linear(self.in_dim if l == 0 else hidden_dim, 3 if l == num_layers - 1 else hidden_dim, bias=False)
            for l in range(num_layers))
        self.bg_net = None
        self._register_state_dict_hook(self._to_reference_layout)
        self._register_load_state_dict_pre_hook(self._from_reference_layout)

    def _init_set(self, ranks, scale=0.1):
        """Planes [H, W, R] and lines [D, R], N(0, scale^2)."""
        res = self.resolution
        mat = [nn.Parameter(scale * torch.randn(res[m1], res[m0], ranks[i])) for i, (m0, m1) in enumerate(MAT_IDS)]
        vec = [nn.Parameter(scale * torch.randn(res[VEC_IDS[i]], ranks[i])) for i in range(3)]
        return nn.ParameterList(mat), nn.ParameterList(vec)

    # ------------------------------------------------------- reference-layout state
    @staticmethod
    def _to_reference_layout(module, state, prefix, local_metadata):
        for name in _SETS:
            conv = plane_to_ref if name.endswith("mat") else line_to_ref
            for i in range(3):
                key = f"{prefix}{name}.{i}"
                if key in state:
                    state[key] = conv(state[key])

    def _from_reference_layout(self, state, prefix, local_metadata, strict, missing, unexpected, errors):
        """Reference-layout entries become [H, W, R] / [D, R]; a parameter of
        another resolution is reallocated to the entry's shape first."""
        for name in _SETS:
            conv = plane_from_ref if name.endswith("mat") else line_from_ref
            params = getattr(self, name)
            for i in range(3):
                key = f"{prefix}{name}.{i}"
                if key not in state:
                    continue
                if state[key].dim() == 4:
                    state[key] = conv(state[key])
                if state[key].shape != params[i].shape and state[key].shape[-1] == params[i].shape[-1]:
                    params[i] = nn.Parameter(torch.empty(state[key].shape, dtype=params[i].dtype,
                                                         device=params[i].device))
        self._resolution_from_params()

    def _resolution_from_params(self):
        for i, (m0, m1) in enumerate(MAT_IDS):
            self.resolution[m1], self.resolution[m0] = int(self.sigma_mat[i].shape[0]), int(self.sigma_mat[i].shape[1])

    # ------------------------------------------------------------------ the field
    def _vm(self, x, sigma=True, color=True):
        """x in world units -> (the density set's sum | None, the colour set's products | None): one kernel call."""
        return vm_sample(x, self.aabb_train, (list(self.sigma_mat), list(self.sigma_vec)) if sigma else None,
                         (list(self.color_mat), list(self.color_vec)) if color else None)

    def _rgb(self, prod, d):
        h = torch.cat([self.encoder(self.basis_mat(prod)), self.encoder_dir(d)], dim=-1)
        for l in range(self.num_layers):
            h = self.color_net[l](h)
            if l != self.num_layers - 1:
                h = F.relu(h, inplace=True)
        return torch.sigmoid(h)

    def forward(self, x, d):
        """x [N, 3] in [-bound, bound], d [N, 3] unit -> (sigma [N], rgb [N, 3])."""
        sigma_feat, prod = self._vm(x)
        return trunc_exp(sigma_feat), self._rgb(prod, d)

    def density(self, x):
        sigma_feat, _ = self._vm(x, color=False)
        return {"sigma": trunc_exp(sigma_feat)}

    def color(self, x, d, mask=None, **kwargs):
        """rgb [N, 3]; with mask [N] bool only where it is set (zeros elsewhere)."""
        if mask is not None:
            rgbs = torch.zeros(mask.shape[0], 3, dtype=x.dtype, device=x.device)
            if not mask.any():
                return rgbs
            x, d = x[mask], d[mask]
        _, prod = self._vm(x, sigma=False)
        h = self._rgb(prod, d)
        if mask is None:
            return h
        rgbs[mask] = h.to(rgbs.dtype)
        return rgbs

    def _query_density(self, xyzs, indices, tmp_grid):
        """The density update's query: the sum kernel alone, no autograd."""
        sigma_feat, _ = self._vm(xyzs.detach().float(), color=False)
        sigmas = torch.exp(sigma_feat.detach()) * self.density_scale
        tmp_grid.view(-1).view(torch.int32).scatter_reduce_(0, indices.long(), sigmas.view(torch.int32), "amax")

    def density_loss(self):
        """The L1 penalty: mean |.| over every density plane and line."""
        loss = 0
        for i in range(3):
            loss = loss + self.sigma_mat[i].abs().mean() + self.sigma_vec[i].abs().mean()
        return loss

    # -------------------------------------------------------- upsample and shrink
    @torch.no_grad()
    def upsample_model(self, resolution):
        """Every plane and line resampled to `resolution` (bilinear,
        align_corners=True): F.interpolate on the reference-layout view."""
        resolution = [int(r) for r in resolution]
        for mats, vecs in ((self.sigma_mat, self.sigma_vec), (self.color_mat, self.color_vec)):
            for i, (m0, m1) in enumerate(MAT_IDS):
                mats[i] = nn.Parameter(plane_from_ref(F.interpolate(
                    plane_to_ref(mats[i].data), size=(resolution[m1], resolution[m0]), mode="bilinear",
                    align_corners=True)))
                vecs[i] = nn.Parameter(line_from_ref(F.interpolate(
                    line_to_ref(vecs[i].data), size=(resolution[VEC_IDS[i]], 1), mode="bilinear",
                    align_corners=True)))
        self.resolution = resolution

    @torch.no_grad()
    def shrink_model(self, log=None):
        """aabb_train and every plane and line cropped to the occupied cells of
        the coarsest density grid (tensoRF/network.py:283-318): the cells above
        min(density_thresh, mean_density), their centres' bounding box grown by
        half a cell, rounded to texels of the current box. An empty grid
        changes nothing. -> (tl, br), the slice kept per axis."""
        half = self.bound / self.grid_size
        thresh = min(self.density_thresh, self.mean_density)
        cells = torch.nonzero(self.density_grid[self.cascade - 1] > thresh).reshape(-1)
        if cells.numel() == 0:
            return None
        pos = morton3D_invert(cells)
        pos = (2 * pos / (self.grid_size - 1) - 1) * (self.bound - half)  # cell centres
        lo, hi = pos.amin(0) - half, pos.amax(0) + half
        aabb = self.aabb_train
        reso = torch.tensor(self.resolution, dtype=torch.long, device=aabb.device)
        units = (aabb[3:] - aabb[:3]) / reso
        tl = torch.round((lo - aabb[:3]) / units).long().clamp(min=0)
        br = torch.minimum(torch.round((hi - aabb[:3]) / units).long(), reso)
        tl, br = tl.tolist(), br.tolist()
        for mats, vecs in ((self.sigma_mat, self.sigma_vec), (self.color_mat, self.color_vec)):
            for i, (m0, m1) in enumerate(MAT_IDS):
                v = VEC_IDS[i]
                vecs[i] = nn.Parameter(vecs[i].data[tl[v]:br[v]].contiguous())
                mats[i] = nn.Parameter(mats[i].data[tl[m1]:br[m1], tl[m0]:br[m0]].contiguous())
        self.aabb_train = torch.cat([lo, hi]).to(aabb.dtype)
        self.resolution = [br[a] - tl[a] for a in range(3)]
        if log:
            log(f"[INFO] shrink slice: {tl} - {br}; new aabb: {self.aabb_train.tolist()}")
        return tl, br

    def get_params(self, lr0, lr1):
        """lr0 for the planes and lines, lr1 for basis_mat and the MLP."""
        return [{"params": list(self.sigma_mat), "lr": lr0}, {"params": list(self.sigma_vec), "lr": lr0},
                {"params": list(self.color_mat), "lr": lr0}, {"params": list(self.color_vec), "lr": lr0},
                {"params": list(self.basis_mat.parameters()), "lr": lr1},
                {"params": list(self.color_net.parameters()), "lr": lr1}]

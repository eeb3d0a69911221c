"""Signed distance fields of triangle meshes (the reference's sdf/ package and
main_sdf.py) on the hash-grid and fully-fused-MLP core. DESIGN.md §21."""
from .loss import mape, mape_loss
from .network_ff import SDFNetwork
from .provider import (MeshSDF, SDFDataset, mesh_sdf_volume, morton_perm, new_counter, prepare_mesh, read_mesh,
                       read_obj, sdf_query, sdf_sample)
from .utils import SDFTrainer, seed_everything

__all__ = ["MeshSDF", "SDFDataset", "SDFNetwork", "SDFTrainer", "mape", "mape_loss", "mesh_sdf_volume",
           "morton_perm", "new_counter", "prepare_mesh", "read_mesh", "read_obj", "sdf_query", "sdf_sample",
           "seed_everything"]

"""TensoRF fields (the reference's tensoRF/ package and main_tensoRF.py): the
vector-matrix decomposition sampled by csrc/tensorf.hip, marched, composited
and pruned by the NeRFRenderer and raymarching operators. DESIGN.md §22."""
from .network import NeRFNetwork, morton3D_invert, upsample_resolution, upsample_schedule
from .utils import TensoRFTrainer, seed_everything
from .vm import (MAT_IDS, VEC_IDS, line_from_ref, line_to_ref, plane_from_ref, plane_to_ref, vm_quantum,
                 vm_reference, vm_sample)

__all__ = ["MAT_IDS", "NeRFNetwork", "TensoRFTrainer", "VEC_IDS", "line_from_ref", "line_to_ref", "morton3D_invert",
           "plane_from_ref", "plane_to_ref", "seed_everything", "upsample_resolution", "upsample_schedule",
           "vm_quantum", "vm_reference", "vm_sample"]

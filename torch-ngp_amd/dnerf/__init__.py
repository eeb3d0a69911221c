"""D-NeRF (the reference's dnerf/ package and main_dnerf.py): a deformation
network in front of the hash-grid field, a time per frame, and one occupancy
grid per time slice updated on the device (csrc/dnerf.hip). DESIGN.md §23."""
from .backend import ENCODE_COLS, encode, grid_ema_pack, grid_points, grid_points_workspace
from .network import NeRFNetwork
from .provider import NeRFDataset, frame_time, normalize_times
from .renderer import NeRFRenderer
from .utils import DNeRFTrainer, seed_everything

__all__ = ["DNeRFTrainer", "ENCODE_COLS", "NeRFDataset", "NeRFNetwork", "NeRFRenderer", "encode", "frame_time",
           "grid_ema_pack", "grid_points", "grid_points_workspace", "normalize_times", "seed_everything"]

"""D-NeRF dataset (reference dnerf/provider.py:228-254, 326-333): the static
nerf.provider.NeRFDataset plus a time per frame. A frame's time is its 'time'
entry when present, otherwise the integer in its file name (the frame index);
when the largest time exceeds 1 all are divided by max + 1e-8. `times` is
float32 [n, 1] on the device and a batch carries 'time' [1, 1], its frame's."""
import json
import os

import numpy as np
import torch

from nerf.provider import NeRFDataset as _StaticDataset


def frame_time(frame):
    """frame['time'], or the integer of the file name without its extension (reference :237-241)."""
    if "time" in frame:
        return float(frame["time"])
    stem = os.path.splitext(os.path.basename(frame["file_path"]))[0]
    try:
        return float(int(stem))
    except ValueError:
        raise ValueError(f"dnerf provider: frame {frame['file_path']!r} has no 'time' and its file name is not an "
                         "integer") from None


def normalize_times(times):
    """float32 [n, 1]; divided by max + 1e-8 when the largest exceeds 1 (reference :250-254)."""
    times = np.asarray(times, dtype=np.float32).reshape(-1, 1)
    if times.size and times.max() > 1:
        times = times / (times.max() + 1e-8)
    return times.astype(np.float32)


def _frames(path, type):
    """The frames NeRFDataset loads, in its order."""
    if os.path.exists(os.path.join(path, "transforms.json")):
        with open(os.path.join(path, "transforms.json")) as f:
            return json.load(f)["frames"]
    frames = []
    for sp in (["train", "val"] if type == "trainval" else [type]):
        with open(os.path.join(path, f"transforms_{sp}.json")) as f:
            frames += json.load(f)["frames"]
    return frames


class NeRFDataset(_StaticDataset):
    def __init__(self, path, device, type="train", **kwargs):
        super().__init__(path, device, type=type, **kwargs)
        times = normalize_times([frame_time(fr) for fr in _frames(path, type)])
        if times.shape[0] != self.poses.shape[0]:
            raise RuntimeError(f"dnerf provider: {times.shape[0]} times for {self.poses.shape[0]} frames")
        self.times = torch.from_numpy(times).to(device)

    def sample(self, index=None, generator=None):
        out = super().sample(index, generator)
        i = out["index"]
        out["time"] = self.times[i:i + 1]
        return out

"""mape_loss (the reference's loss.py) on the device: csrc/sdf.hip ngp_sdf_mape."""
import torch
from torch.autograd import Function

import _ngp_native as nat

MAPE_BLOCKS = 256  # include/ngp_hip.h NGP_SDF_MAPE_BLOCKS


def _check(pred, y):
    nat.check_tensor(pred, "pred", dtypes=(torch.float32, torch.float16), what="float32 or float16")
    nat.check_tensor(y, "y", dtypes=(torch.float32,), what="float32")
    if pred.numel() != y.numel() or pred.numel() == 0:
        raise RuntimeError("pred and y must hold the same, non-zero number of elements")


def mape(pred, y, grad=True, grad_scale=None):
    """mean(|pred - y| / (|y| + 1e-2)) as a float64 device scalar, and dL/dpred
    in pred's dtype (None without grad), times the device float grad_scale when
    one is given. One pass over the elements and a fixed summation order."""
    _check(pred, y)
    dev, n = pred.device, pred.numel()
    partials = torch.empty(MAPE_BLOCKS, dtype=torch.float64, device=dev)
    loss = torch.empty((), dtype=torch.float64, device=dev)
    g = torch.empty_like(pred) if grad else None
    P = nat.ptr
    nat.check(nat.lib().ngp_sdf_mape(P(pred), nat.DTYPE_CODE[pred.dtype], P(y), n, P(grad_scale), P(g), P(partials),
                                     P(loss), nat.stream_of(pred)), "sdf_mape")
    return loss, g


class _mape_loss(Function):
    @staticmethod
    def forward(ctx, pred, y):
        pred_c, y_c = pred.contiguous(), y.contiguous()
        loss, _ = mape(pred_c, y_c, grad=False)
        ctx.save_for_backward(pred_c, y_c)
        return loss.float()

    @staticmethod
    def backward(ctx, grad_out):
        # the gradient times the incoming one (GradScaler's scale) before it is rounded to pred's dtype
        pred_c, y_c = ctx.saved_tensors
        scale = grad_out.detach().float().reshape(1).contiguous()
        _, g = mape(pred_c, y_c, grad=True, grad_scale=scale)
        return g, None


def mape_loss(pred, y):
    """The reference's criterion as an autograd op: a float32 scalar."""
    return _mape_loss.apply(pred, y)

"""`_backend` for shencoder (reference shencoder/src/bindings.cpp:5-8,
shencoder.h:9-10) bound to libngp_hip.so via ctypes."""
import types

import torch

import _ngp_native as nat

_F = (torch.float32, torch.float64)


def _check_dims(what, B, D, C):
    for v, n in ((B, "B"), (D, "D"), (C, "C")):
        if not isinstance(v, int) or v < 0:
            raise RuntimeError(f"{what}: {n} must be a non-negative int, got {v!r}")


def _check_args(what, B, D, C, tensors):
    """The kernels take raw pointers and one element type for all of them
    (the reference's AT_DISPATCH with data_ptr<scalar_t>() raises on a
    mismatch, shencoder.cu:400-439): every tensor must be float32/float64 of
    the first one's dtype, on its device, and hold what B, D, C index.
    `tensors` is (tensor, name, elements needed); the first sets the type."""
    first, first_name, _ = tensors[0]
    for t, name, need in tensors:
        nat.check_tensor(t, name, _F, "float32/float64")
        if t.dtype != first.dtype:
            raise RuntimeError(f"{what}: {name} is {t.dtype} but {first_name} is {first.dtype}; "
                               "all tensors must have one dtype")
        if t.device != first.device:
            raise RuntimeError(f"{what}: {name} is on {t.device} but {first_name} is on {first.device}")
        if t.numel() < need:
            raise RuntimeError(f"{what}: {name} has {t.numel()} elements, B, D, C = {B}, {D}, {C} "
                               f"need {need}")


def sh_encode_forward(inputs, outputs, B, D, C, dy_dx):
    _check_dims("sh_encode_forward", B, D, C)
    tensors = [(inputs, "inputs", B * D), (outputs, "outputs", B * C * C)]
    if dy_dx is not None:
        tensors.append((dy_dx, "dy_dx", B * D * C * C))
    _check_args("sh_encode_forward", B, D, C, tensors)
    nat.check(nat.lib().ngp_sh_encode_forward(nat.ptr(inputs), nat.ptr(outputs), B, D, C,
                                              nat.ptr(dy_dx), nat.DTYPE_CODE[inputs.dtype],
                                              nat.stream_of(inputs)), "sh_encode_forward")


def sh_encode_backward(grad, inputs, B, D, C, dy_dx, grad_inputs):
    _check_dims("sh_encode_backward", B, D, C)
    _check_args("sh_encode_backward", B, D, C,
                [(grad, "grad", B * C * C), (inputs, "inputs", B * D),
                 (dy_dx, "dy_dx", B * D * C * C), (grad_inputs, "grad_inputs", B * D)])
    nat.check(nat.lib().ngp_sh_encode_backward(nat.ptr(grad), nat.ptr(inputs), B, D, C,
                                               nat.ptr(dy_dx), nat.ptr(grad_inputs),
                                               nat.DTYPE_CODE[grad.dtype], nat.stream_of(grad)),
              "sh_encode_backward")


_backend = types.SimpleNamespace(sh_encode_forward=sh_encode_forward,
                                 sh_encode_backward=sh_encode_backward)

__all__ = ["_backend"]

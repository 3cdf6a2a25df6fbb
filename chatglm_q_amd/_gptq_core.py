"""What the int4g32 and the int8 GPTQ quantizers share (chatglm_q/int4/quantizer.py:78-196, chatglm_q/int8/quantizer.py:55-164):
the Hessian hook, dead columns, damping, the two Cholesky factorisations and the walk over blocks of input columns.

GPTQ: https://arxiv.org/abs/2210.17323, https://github.com/IST-DASLab/gptq (Apache License 2.0).

The walk inside a block is ``fused_ops.gptq_block`` - one launch of csrc/gptq.hip per block on a GPU, the reference's
column-by-column torch loop elsewhere.  The update of the columns right of a block, the Hessian accumulation and the
factorisations are torch calls on the weight's device (fp32, no TF32)."""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import Tensor, nn

from . import fused_ops


# None: the HIP kernel when the weight is a contiguous float32 tensor on a GPU, the composed torch formula otherwise.  A plain module
# attribute like the route switches of model.py: what a quantizer takes when its caller passes no ``use_kernel`` (the model-level
# driver passes none), so tests and tools/gptq_bench.py can send a whole run down either path.
USE_KERNEL: Optional[bool] = None


class GPTQQuantizerBase:
    bits = 0            # 4 / 8, set by the subclasses

    def __init__(self, layer: nn.Module):
        if not isinstance(layer, nn.Linear):
            raise AssertionError("expected nn.Linear")
        self.layer = layer
        self.hook = layer.register_forward_hook(self.forward_hook)
        self.n_rows, self.n_columns = layer.weight.shape        # output_dim, input_dim
        self.hessian = torch.zeros((self.n_columns, self.n_columns), device=layer.weight.device)
        self.n_samples = 0
        self.debug_input = None

    @torch.no_grad()
    def forward_hook(self, module: nn.Module, inputs: tuple, output: Tensor):
        """Running mean of 2 x x^T over every input row the layer has seen."""
        input, = inputs
        if input.dim() > 2:
            input = input.flatten(0, -2)
        self.debug_input = input.detach()
        new_samples, d_hidden = input.shape
        if d_hidden != self.n_columns:
            raise AssertionError(f"input of {d_hidden} features for a layer of {self.n_columns}")
        self.hessian *= self.n_samples / (self.n_samples + new_samples)
        self.n_samples += new_samples
        x = math.sqrt(2 / self.n_samples) * input.t().float()
        self.hessian += x.matmul(x.t())

    def remove_hook(self):
        self.hook.remove()

    def _factor(self, weight: Tensor, percdamp: float) -> Tensor:
        """Zero the dead columns of ``weight``, damp the Hessian (in place, as the reference does) and return the upper Cholesky
        factor of its inverse."""
        hessian = self.hessian
        dead = torch.diag(hessian) == 0
        hessian[dead, dead] = 1
        weight[:, dead] = 0
        damp = percdamp * torch.mean(torch.diag(hessian))
        diag = torch.arange(self.n_columns, device=weight.device)
        hessian[diag, diag] += damp
        hinv = torch.cholesky_inverse(torch.linalg.cholesky(hessian))
        hinv = torch.linalg.cholesky(hinv, upper=True)
        if hinv.isnan().any():
            raise AssertionError("the Cholesky factor of the inverse Hessian holds NaN")
        return hinv

    def _walk(self, weight: Tensor, hinv: Tensor, scale: Tensor, blocksize: int, group: int, use_kernel: Optional[bool]):
        """Block by block over the input columns.  Returns (grid_weight, mean of the loss terms)."""
        if not 1 <= blocksize <= fused_ops.GPTQ_MAX_BLOCK:
            raise ValueError(f"blocksize must be in [1, {fused_ops.GPTQ_MAX_BLOCK}], got {blocksize}")
        if use_kernel is None:
            use_kernel = USE_KERNEL
        if use_kernel is None:
            use_kernel = weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()
        elif use_kernel and not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()):
            raise ValueError("use_kernel=True needs a contiguous float32 weight on a GPU")
        hinv_rows = hinv.contiguous()         # linalg.cholesky(upper=True) returns a transposed view; the walk reads rows
        grid_weight = torch.empty_like(weight)
        loss_sum = torch.zeros((), dtype=torch.float64, device=weight.device)
        for i1 in range(0, self.n_columns, blocksize):
            i2 = min(i1 + blocksize, self.n_columns)
            Q, Err, Loss = fused_ops.gptq_block(weight, i1, i2 - i1, hinv_rows, self.bits, scale, group, use_kernel=use_kernel)
            grid_weight[:, i1:i2] = Q
            loss_sum += Loss.sum(dtype=torch.float64)
            if i2 < self.n_columns:
                weight[:, i2:] -= Err.matmul(hinv[i1:i2, i2:])
        return grid_weight, loss_sum.item() / max(1, weight.numel())

    def _debug_loss(self, grid_weight: Tensor) -> float:
        debug_output = nn.functional.linear(self.debug_input, self.layer.weight)
        quant_out = nn.functional.linear(self.debug_input, grid_weight.type_as(self.layer.weight))
        return torch.mean((quant_out - debug_output) ** 2).item()

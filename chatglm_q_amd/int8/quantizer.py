"""int8 per-row quantisers: the writers of the int8 buffer format (chatglm_q/int8/quantizer.py).

Round to nearest (``quantize_int8``, ``get_quant_int8_linear``, ``get_quant_embedding``) and GPTQ (``GPTQLinearQuantizer``,
``clamp_to_quantize_grid``, ``quantize_with_scale``; chatglm_q/int8/quantizer.py:22-30,55-164): calibrated quantisation of an
``nn.Linear`` from the inputs it sees, the walk inside a block of input columns being one launch of csrc/gptq.hip on a GPU
(chatglm_q_amd/_gptq_core.py); ``chatglm_q_amd.gptq`` drives it over a whole model."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .._gptq_core import GPTQQuantizerBase
from .qlinear import DynamicQuantizeLinear, QEmbedding

max_q_int8 = 2 ** (8 - 1) - 1  # 127


@torch.no_grad()
def quantize_int8(inputs: Tensor):
    """Row-wise symmetric: weights (out, in) or activations (channels, features).
    scale = clamp(max|row| / 127, min=1e-10); q = clamp(round(x / scale), -127, 127)."""
    scale = torch.clamp(inputs.abs().amax(dim=1, keepdim=True) / max_q_int8, min=1e-10)
    q = torch.clamp(torch.round(inputs / scale), -max_q_int8, max_q_int8)
    return q.to(torch.int8), scale.squeeze(dim=-1)


@torch.no_grad()
def get_quant_int8_linear(layer: nn.Linear):
    if not isinstance(layer, nn.Linear):
        raise AssertionError("expected nn.Linear")
    q_weight, scale = quantize_int8(layer.weight)
    out = DynamicQuantizeLinear(layer.in_features, layer.out_features, layer.bias is not None,
                                device=layer.weight.device, dtype=layer.weight.dtype)
    out.apply_weights_(q_weight, scale, layer.bias)
    return out


@torch.no_grad()
def get_quant_embedding(layer: nn.Embedding):
    if not isinstance(layer, nn.Embedding):
        raise AssertionError("expected nn.Embedding")
    q_weight, scale = quantize_int8(layer.weight.t())
    out = QEmbedding(layer.num_embeddings, layer.embedding_dim, device=layer.weight.device, dtype=layer.weight.dtype)
    out.apply_weights_(q_weight.t(), scale)
    return out


@torch.no_grad()
def clamp_to_quantize_grid(x: Tensor, scale: Tensor) -> Tensor:
    """The nearest value to ``x`` on the int8 grid of ``scale``: scale * clamp(round(x / scale), -127, 127)."""
    return scale * torch.clamp(torch.round(x / scale), -max_q_int8, max_q_int8)


@torch.no_grad()
def quantize_with_scale(x: Tensor, scale: Tensor) -> Tensor:
    """int8 codes of ``x`` for a GIVEN (broadcastable) scale."""
    return torch.clamp(torch.round(x / scale), -max_q_int8, max_q_int8).to(torch.int8)


class GPTQLinearQuantizer(GPTQQuantizerBase):
    """GPTQ for one ``nn.Linear`` into the int8 per-row format (chatglm_q/int8/quantizer.py:55-164).  Constructing it hooks the
    layer; every forward of the layer then adds its inputs to the Hessian estimate; ``get_quantized_linear`` returns the
    replacement module.  The row scales come from the ORIGINAL weights and stay fixed during the walk."""
    bits = 8

    @torch.no_grad()
    def quantize_weight(self, blocksize=128, percdamp=.01, use_kernel: Optional[bool] = None):
        """Returns (grid_weight (out, in), scale (out), quant_losses, debug_loss).  ``use_kernel``: None - the HIP kernel when the
        weight is a contiguous float32 tensor on a GPU, the composed torch formula otherwise; True / False force either."""
        if self.n_samples <= 0:
            raise AssertionError("no calibration input has passed through the layer")
        weight = self.layer.weight.detach().clone()
        _, scale = quantize_int8(weight)
        scale = scale.contiguous()
        hinv = self._factor(weight, percdamp)
        grid_weight, quant_losses = self._walk(weight, hinv, scale, blocksize, 0, use_kernel)
        return grid_weight, scale, quant_losses, self._debug_loss(grid_weight)

    @torch.no_grad()
    def get_quantized_linear(self, blocksize=128, percdamp=.01, pring_loss=False, use_kernel: Optional[bool] = None):
        grid_weight, scale, quant_losses, debug_loss = self.quantize_weight(blocksize, percdamp, use_kernel=use_kernel)
        if pring_loss:
            print(f"{quant_losses=:.8f} {debug_loss=:.8f}")
        original = self.layer
        modified = DynamicQuantizeLinear(original.in_features, original.out_features, original.bias is not None,
                                         device=original.weight.device, dtype=original.weight.dtype)
        modified.apply_weights_(quantize_with_scale(grid_weight, scale[:, None]), scale, original.bias)
        return modified

"""int4 group quantisers: the WRITERS of the buffer format the kernels consume (chatglm_q/int4/quantizer.py).

Round to nearest (``quantize_int4``, ``get_quant_int4_linear``, ``get_quant_embedding``): used to synthesise weights for
benchmarks and to convert ``nn.Linear`` / ``nn.Embedding`` layers.  GPTQ (``GPTQLinearQuantizer``, ``clamp_to_quantize_grid``,
``quantize_with_scale``; chatglm_q/int4/quantizer.py:32-53,78-196): calibrated quantisation of an ``nn.Linear`` from the inputs it
sees, the walk inside a block of input columns being one launch of csrc/gptq.hip on a GPU (chatglm_q_amd/_gptq_core.py);
``chatglm_q_amd.gptq`` drives it over a whole model."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from . import qlinear
from .._gptq_core import GPTQQuantizerBase
from .qlinear import DynamicQuantizeLinear, QEmbedding

max_q_int4 = 2 ** (4 - 1) - 1  # 7


@torch.no_grad()
def quantize_int4(x: Tensor, GROUP_K: int = qlinear.DEFAULT_GROUP_SIZE):
    """x: (in_dim, out_dim) weight.  Returns (packed (in/2, out) uint8, scale (in/GROUP_K, out)).

    Per group: scale = clamp(max|x| / 7, min=1e-10); q = clamp(round(x / scale), -7, 7) (round half to
    even); stored nibble = q + 8; two K rows per byte, even row in the low nibble.
    """
    if x.dim() != 2:
        raise AssertionError("expected a 2-D weight")
    K, N = x.shape
    if K % GROUP_K != 0:
        raise AssertionError(f"K={K} not divisible by group {GROUP_K}")
    G = K // GROUP_K
    xg = x.reshape(G, GROUP_K, N)
    scale = torch.clamp(xg.abs().amax(dim=1, keepdim=True) / max_q_int4, min=1e-10)
    q = torch.clamp(torch.round(xg / scale), -max_q_int4, max_q_int4)
    q = (q + 8).to(torch.uint8).reshape(K, N)
    packed = (q[0::2] & 0xF) | ((q[1::2] & 0xF) << 4)
    return packed.contiguous(), scale.reshape(G, N)


@torch.no_grad()
def get_quant_int4_linear(layer: nn.Linear, group_size: int = qlinear.DEFAULT_GROUP_SIZE):
    if not isinstance(layer, nn.Linear):
        raise AssertionError("expected nn.Linear")
    q_weight, scale = quantize_int4(layer.weight.t(), group_size)
    out = DynamicQuantizeLinear(layer.in_features, layer.out_features, layer.bias is not None, group_size,
                                device=layer.weight.device, dtype=layer.weight.dtype)
    out.apply_weights_(q_weight, scale, layer.bias)
    return out


@torch.no_grad()
def get_quant_embedding(layer: nn.Embedding, group_size: int = qlinear.DEFAULT_GROUP_SIZE):
    if not isinstance(layer, nn.Embedding):
        raise AssertionError("expected nn.Embedding")
    q_weight, scale = quantize_int4(layer.weight, group_size)
    out = QEmbedding(layer.num_embeddings, layer.embedding_dim, group_size,
                     device=layer.weight.device, dtype=layer.weight.dtype)
    out.apply_weights_(q_weight, scale)
    return out


@torch.no_grad()
def clamp_to_quantize_grid(x: Tensor, scale: Tensor) -> Tensor:
    """The nearest value to ``x`` on the int4 grid of ``scale``: scale * clamp(round(x / scale), -7, 7)."""
    return scale * torch.clamp(torch.round(x / scale), -max_q_int4, max_q_int4)


@torch.no_grad()
def quantize_with_scale(x: Tensor, scale: Tensor) -> Tensor:
    """x: (in_dim, out_dim) weight, scale (in_dim / group, out_dim) GIVEN.  Returns the packed (in/2, out) uint8 codes of
    ``quantize_int4``'s format: nibble = clamp(round(x / scale), -7, 7) + 8, even row in the low nibble."""
    if x.dim() != 2 or scale.dim() != 2:
        raise AssertionError("expected a 2-D weight and a 2-D scale")
    K, N = x.shape
    G = scale.shape[0]
    if K % G != 0:
        raise AssertionError(f"K={K} not divisible into {G} groups")
    q = torch.clamp(torch.round(x.reshape(G, K // G, N) / scale.reshape(G, 1, N)), -max_q_int4, max_q_int4)
    q = (q + 8).to(torch.uint8).reshape(K, N)
    return (q[0::2] & 0xF) | ((q[1::2] & 0xF) << 4)


class GPTQLinearQuantizer(GPTQQuantizerBase):
    """GPTQ for one ``nn.Linear`` into the int4 group format (chatglm_q/int4/quantizer.py:78-196).  Constructing it hooks the
    layer; every forward of the layer then adds its inputs to the Hessian estimate; ``get_quantized_linear`` returns the
    replacement module.  The scale of a group is taken when the walk reaches the group, from the weights as updated so far."""
    bits = 4

    @torch.no_grad()
    def quantize_weight(self, blocksize=128, groupsize=qlinear.DEFAULT_GROUP_SIZE, percdamp=.01, use_kernel: Optional[bool] = None):
        """Returns (grid_weight (out, in), scale (in / groupsize, out), quant_losses, debug_loss).  ``use_kernel``: None - the
        HIP kernel when the weight is a contiguous float32 tensor on a GPU, the composed torch formula otherwise; True / False
        force either."""
        if self.n_samples <= 0:
            raise AssertionError("no calibration input has passed through the layer")
        if blocksize % groupsize != 0:
            raise AssertionError(f"{blocksize=}, {groupsize=}")
        if self.n_columns % groupsize != 0:
            raise AssertionError(f"{self.n_columns=}, {groupsize=}")
        weight = self.layer.weight.detach().clone()
        hinv = self._factor(weight, percdamp)
        scale = torch.empty((self.n_columns // groupsize, self.n_rows), dtype=weight.dtype, device=weight.device)
        grid_weight, quant_losses = self._walk(weight, hinv, scale, blocksize, groupsize, use_kernel)
        return grid_weight, scale, quant_losses, self._debug_loss(grid_weight)

    @torch.no_grad()
    def get_quantized_linear(self, blocksize=128, groupsize=qlinear.DEFAULT_GROUP_SIZE, percdamp=.01, pring_loss=False,
                             use_kernel: Optional[bool] = None):
        grid_weight, scale, quant_losses, debug_loss = self.quantize_weight(blocksize, groupsize, percdamp, use_kernel=use_kernel)
        if pring_loss:
            print(f"{quant_losses=:.8f} {debug_loss=:.8f}")
        original = self.layer
        modified = DynamicQuantizeLinear(original.in_features, original.out_features, original.bias is not None, groupsize,
                                         device=original.weight.device, dtype=original.weight.dtype)
        modified.apply_weights_(quantize_with_scale(grid_weight.t(), scale), scale, original.bias)
        return modified

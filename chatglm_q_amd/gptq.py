"""GPTQ over a whole float ``ChatGLM2Model`` (the flow of the reference's examples/quantize_gptq/int4g32.py:41-104 and int8.py).

    from chatglm_q_amd.gptq import gptq_quantize_model_
    gptq_quantize_model_(model, batches, quant_type="int4g32", device="cuda")
    save_model(folder, ChatGLMLoadConfig(model_config=model.config, quant_type="int4g32", torch_dtype="float16"), model)

The embedding is quantised round to nearest.  Then block by block: every ``nn.Linear`` of the block gets a
``GPTQLinearQuantizer``, the block runs over the calibration hidden states that the earlier - already quantised - blocks
produced, and the linears are replaced.  ``final_ln`` + ``lm_head`` go last.  Each block is moved to ``device`` for its turn and
back, so a model that does not fit the GPU as float32 still calibrates there; on a GPU the walk inside every block of 128 input
columns is one launch of csrc/gptq.hip."""
from __future__ import annotations

from typing import Callable, Iterable, Optional

import torch
from torch import nn

from .model import ChatGLM2Model


def _prepare(model: ChatGLM2Model, input_ids, attention_mask=None):
    """Embeddings, additive mask and rotary table rows of one calibration batch (ChatGLM2Model.forward's preamble)."""
    h = model.word_embedding(input_ids)
    B, S, _ = h.shape
    if attention_mask is None:
        attention_mask = torch.ones(B, S, dtype=torch.long, device=h.device)
    position_ids = torch.cumsum(attention_mask, dim=1)
    t = torch.arange(S, device=h.device)
    blocked = (t[:, None] < t[None, :])[None] | ~attention_mask[:, None, :].bool()
    return h, blocked.float() * -1e10, model._rotary(position_ids)


def _run_block(layer, h, mask, cs):
    q, k, v = layer.attn.project(layer.attn_ln(h), cs)
    h = h + layer.attn.attend(h.dtype, q, k, v, mask)
    return h + layer.ffn(layer.ffn_ln(h))


def _replace_linears(root: nn.Module, run: Callable[[], None], quantizer_cls, blocksize, percdamp, log, prefix):
    """Hook every nn.Linear under ``root``, call ``run()`` (which must push the calibration data through them), swap them."""
    quantizers = {name: quantizer_cls(m) for name, m in root.named_modules() if isinstance(m, nn.Linear)}
    run()
    for name, q in quantizers.items():
        q.remove_hook()
        parent_path, _, leaf = name.rpartition(".")
        parent = root.get_submodule(parent_path) if parent_path else root
        setattr(parent, leaf, q.get_quantized_linear(blocksize=blocksize, percdamp=percdamp))
        if log is not None:
            log(f"{prefix}{name}: {q.n_rows} x {q.n_columns}, {q.n_samples} samples")


@torch.no_grad()
def gptq_quantize_model_(model: ChatGLM2Model, batches: Iterable[dict], quant_type: str = "int4g32", device=None, blocksize: int = 128,
                         percdamp: float = .01, log: Optional[Callable[[str], None]] = None) -> ChatGLM2Model:
    """Quantise a float ``ChatGLM2Model`` in place with GPTQ and return it.  ``batches``: dicts of ``input_ids`` (B, S) and
    optionally ``attention_mask`` (B, S), on the model's device.  ``quant_type``: "int4g32" or "int8".  ``device``: where each
    block is calibrated and quantised (default: where the model is).  ``log``: called with one line per replaced layer.  The
    result has the modules, state_dict keys and dtypes of ``create_quant_int4_model`` / ``create_quant_int8_model``, so it
    saves and loads through chatglm_q_amd.loader."""
    if quant_type == "int4g32":
        from .int4 import quantizer as Q
    elif quant_type == "int8":
        from .int8 import quantizer as Q
    else:
        raise ValueError(f"quant_type must be 'int4g32' or 'int8', got {quant_type!r}")
    home = model.final_ln.weight.device
    device = torch.device(device) if device is not None else home
    model.word_embedding = Q.get_quant_embedding(model.word_embedding)
    prepared = [_prepare(model, **batch) for batch in batches]
    if not prepared:
        raise ValueError("gptq_quantize_model_: no calibration batch")
    hidden = [p[0] for p in prepared]

    for i, layer in enumerate(model.layers):
        layer.to(device)
        out = []

        def run():
            for h, (_, mask, cs) in zip(hidden, prepared):
                out.append(_run_block(layer, h.to(device), mask.to(device), cs.to(device)))

        _replace_linears(layer, run, Q.GPTQLinearQuantizer, blocksize, percdamp, log, f"layers.{i}.")
        hidden = out
        layer.to(home)

    model.final_ln.to(device)
    model.lm_head.to(device)

    def run_head():
        for h in hidden:
            model.lm_head(model.final_ln(h))

    head = nn.ModuleDict({"lm_head": model.lm_head})
    _replace_linears(head, run_head, Q.GPTQLinearQuantizer, blocksize, percdamp, log, "")
    model.lm_head = head["lm_head"]
    model.final_ln.to(home)
    model.lm_head.to(home)
    return model

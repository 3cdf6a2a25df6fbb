"""GPTQ without a GPU: the numpy oracle (tests/_gptq_oracle.py) against the reference's recorded results
(tests/golden/gptq.npz, written by tests/golden/make_golden_gptq.py), the composed torch path of both ``GPTQLinearQuantizer``
classes against the same records, the helpers around them, and ``chatglm_q_amd.gptq.gptq_quantize_model_`` on a tiny float model.

End-to-end conditions (a code flip at a rounding tie changes the rest of that row and no other row, so the comparison goes by
rows): at most max(1, 1 %) of the rows hold a differing integer code; scales of the agreeing rows to rel 1e-5; the
Hessian-weighted error tr((W-Q) H (W-Q)^T) within [0.99, 1.01] of the reference's; quant_losses / debug_loss to rel 1e-5 when
no row differs and rel 1e-2 when one does."""
import numpy as np
import pytest
import torch
from torch import nn

import _golden as G
import _gptq_oracle as GO
from chatglm_q_amd import fused_ops, loader
from chatglm_q_amd.gptq import gptq_quantize_model_
from chatglm_q_amd.int4 import quantizer as q4
from chatglm_q_amd.int8 import quantizer as q8
from chatglm_q_amd.model import ChatGLM2Config, ChatGLM2Model, create_quant_int4_model, create_quant_int8_model

Z = G.load("gptq.npz")
MODS = {"int4": (q4, 4), "int8": (q8, 8)}
TINY = ChatGLM2Config(hidden_size=64, inner_hidden_size=96, head_hidden_size=16, num_multi_query_groups=2, num_attention_heads=4,
                      num_layers=2, vocab_size=96, max_sequence_length=32)


def fixture(name, bits):
    n = GO.CASES[name][1]
    return dict(W=Z[f"{name}/W"], hessian=GO.unpack_symmetric(Z[f"{name}/hessian_packed"], n), n_samples=int(Z[f"{name}/n_samples"]),
                debug_input=Z[f"{name}/debug_input"], hinv=GO.unpack_upper(Z[f"{name}/hessian_inv_packed"], n),
                grid=Z[f"{name}/{bits}/grid_weight"], scale=Z[f"{name}/{bits}/scale"],
                quant_losses=float(Z[f"{name}/{bits}/quant_losses"]), debug_loss=float(Z[f"{name}/{bits}/debug_loss"]))


def armed_quantizer(name, bits, device="cpu"):
    """A quantizer of the package in the state the reference's was in before quantize_weight: the fixture's weight, Hessian,
    sample count and debug input."""
    mod, _ = MODS[bits]
    fx = fixture(name, bits)
    layer = nn.Linear(fx["W"].shape[1], fx["W"].shape[0], bias=False, device=device)
    with torch.no_grad():
        layer.weight.copy_(torch.from_numpy(fx["W"]))
    q = mod.GPTQLinearQuantizer(layer)
    q.remove_hook()
    q.hessian.copy_(torch.from_numpy(fx["hessian"]))
    q.n_samples = fx["n_samples"]
    q.debug_input = torch.from_numpy(fx["debug_input"]).to(device)
    return q, fx


def check_end_to_end(grid, scale, quant_losses, debug_loss, fx, bits, other=None, label=""):
    """The module docstring's conditions, ``(grid, scale, ...)`` against the fixture ``fx`` - or against ``other`` =
    (grid, scale, quant_losses, debug_loss) of another path on the same inputs."""
    nbits = MODS[bits][1]
    ref = (fx["grid"], fx["scale"], fx["quant_losses"], fx["debug_loss"]) if other is None else other
    grid, scale = np.asarray(grid, dtype=np.float32), np.asarray(scale, dtype=np.float32)
    differs = (GO.codes(grid, scale, nbits) != GO.codes(ref[0], ref[1], nbits)).any(axis=1)
    n_rows = grid.shape[0]
    srow = scale if nbits == 8 else scale.T                        # (n_rows, ...) either way
    rrow = ref[1] if nbits == 8 else ref[1].T
    scale_rel = float(np.max(np.abs(srow[~differs] - rrow[~differs]) / rrow[~differs])) if (~differs).any() else 0.0
    ratio = GO.hessian_error(fx["W"], grid, fx["hessian"]) / GO.hessian_error(fx["W"], ref[0], fx["hessian"])
    ql_rel, dl_rel = abs(quant_losses - ref[2]) / ref[2], abs(debug_loss - ref[3]) / ref[3]
    print(f"{label}{bits}: rows differing {int(differs.sum())} of {n_rows}, scale rel {scale_rel:.3g}, error ratio {ratio:.6f}, "
          f"quant_losses rel {ql_rel:.3g}, debug_loss rel {dl_rel:.3g}")
    assert differs.sum() <= max(1, n_rows // 100)
    assert scale_rel <= 1e-5
    assert 0.99 <= ratio <= 1.01
    tol = 1e-2 if differs.any() else 1e-5
    assert ql_rel <= tol and dl_rel <= tol


def rtn_error(fx, bits):
    W = torch.from_numpy(fx["W"])
    if bits == "int4":
        packed, s = q4.quantize_int4(W.t())
        grid = (q4.qlinear.unpack_int4(packed, s)).t()
    else:
        q, s = q8.quantize_int8(W)
        grid = q.float() * s[:, None]
    return GO.hessian_error(fx["W"], grid.numpy(), fx["hessian"])


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_oracle_equals_reference_bitwise(bits):
    # case (a) is one block: no BLAS between the recorded factor and the result
    fx = fixture("a", bits)
    grid, scale, loss, _ = GO.quantize_weight(fx["W"], fx["hessian"], MODS[bits][1], hinv=fx["hinv"])
    assert np.array_equal(grid.view(np.int32), fx["grid"].view(np.int32))
    assert np.array_equal(scale.view(np.int32), fx["scale"].view(np.int32))
    assert abs(loss - fx["quant_losses"]) <= 1e-5 * fx["quant_losses"]


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_host_block_formula_equals_oracle_bitwise(bits):
    # fused_ops.gptq_block off the GPU: torch ops, the same bits as the oracle (first and last block of case b)
    fx = fixture("b", bits)
    nbits = MODS[bits][1]
    W = fx["W"].copy()
    W[:, GO.CASES["b"][2]] = 0
    for c0, bc in ((0, 128), (256, 64)):
        if nbits == 4:
            s_o, s_t = np.zeros((10, 64), np.float32), torch.zeros(10, 64)
        else:
            s_o = np.maximum(np.abs(W).max(axis=1) / np.float32(127), np.float32(1e-10))
            s_t = torch.from_numpy(s_o.copy())
        want = GO.gptq_block(W, c0, bc, fx["hinv"], nbits, s_o)
        got = fused_ops.gptq_block(torch.from_numpy(W), c0, bc, torch.from_numpy(fx["hinv"]), nbits, s_t)
        for w, g in zip(want, got):
            assert np.array_equal(w.view(np.int32), g.numpy().view(np.int32))
        assert np.array_equal(s_o, s_t.numpy())


@pytest.mark.parametrize("bits", ["int4", "int8"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_composed_path_reproduces_reference(name, bits):
    q, fx = armed_quantizer(name, bits)
    grid, scale, quant_losses, debug_loss = q.quantize_weight()
    assert grid.dtype == torch.float32 and tuple(grid.shape) == fx["grid"].shape and tuple(scale.shape) == fx["scale"].shape
    check_end_to_end(grid.numpy(), scale.numpy(), quant_losses, debug_loss, fx, bits, label=f"composed {name}/")
    # ... and it is better than round to nearest in the measure it minimises
    assert GO.hessian_error(fx["W"], grid.numpy(), fx["hessian"]) < rtn_error(fx, bits)


@pytest.mark.parametrize("bits", ["int4", "int8"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_reference_beats_round_to_nearest(name, bits):
    fx = fixture(name, bits)
    ratio = GO.hessian_error(fx["W"], fx["grid"], fx["hessian"]) / rtn_error(fx, bits)
    print(f"{name}/{bits}: GPTQ / round-to-nearest Hessian-weighted error {ratio:.3f}")
    assert ratio < 1.0


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_hessian_accumulation_over_split_batches(bits):
    mod, _ = MODS[bits]
    fx = fixture("b", bits)
    W, batches = GO.calibration_inputs("b")
    assert np.array_equal(W, fx["W"])
    layer = nn.Linear(W.shape[1], W.shape[0], bias=False)
    q = mod.GPTQLinearQuantizer(layer)
    with torch.no_grad():
        for x in batches:
            layer(torch.from_numpy(x))
    assert q.n_samples == fx["n_samples"] and tuple(q.hessian.shape) == fx["hessian"].shape
    assert torch.equal(q.debug_input, torch.from_numpy(fx["debug_input"]))
    # a running mean of fp32 matrix products: BLAS may order the sums differently from the machine that wrote the fixture
    assert np.abs(q.hessian.numpy() - fx["hessian"]).max() <= 1e-5 * np.abs(fx["hessian"]).max()
    dead = GO.CASES["b"][2]
    assert not q.hessian[dead].any() and not q.hessian[:, dead].any()
    q.remove_hook()
    with torch.no_grad():
        layer(torch.from_numpy(batches[0]))
    assert q.n_samples == fx["n_samples"]                       # the hook is gone


def test_quantize_with_scale_packs_like_quantize_int4():
    fx = fixture("b", "int4")
    grid, scale = torch.from_numpy(fx["grid"]), torch.from_numpy(fx["scale"])
    packed = q4.quantize_with_scale(grid.t(), scale)
    assert packed.dtype == torch.uint8 and tuple(packed.shape) == (160, 64)
    code = torch.from_numpy(GO.codes(fx["grid"], fx["scale"], 4)).t() + 8                 # (K, N) nibbles
    assert int(code.min()) >= 1 and int(code.max()) <= 15
    want = ((code[0::2] & 0xF) | ((code[1::2] & 0xF) << 4)).to(torch.uint8)              # quantize_int4's packing
    assert torch.equal(packed, want)
    # a weight that sits on its own round-to-nearest grid packs to quantize_int4's bytes
    rtn_packed, rtn_scale = q4.quantize_int4(torch.from_numpy(fx["W"]).t())
    on_grid = q4.qlinear.unpack_int4(rtn_packed, rtn_scale)
    assert torch.equal(q4.quantize_with_scale(on_grid, rtn_scale), rtn_packed)
    assert torch.equal(q4.clamp_to_quantize_grid(on_grid, rtn_scale.repeat_interleave(32, dim=0)), on_grid)
    # int8
    s8 = torch.from_numpy(fixture("b", "int8")["scale"])
    g8 = torch.from_numpy(fixture("b", "int8")["grid"])
    c8 = q8.quantize_with_scale(g8, s8[:, None])
    assert c8.dtype == torch.int8 and torch.equal(c8.float() * s8[:, None], g8)
    assert torch.equal(q8.clamp_to_quantize_grid(g8, s8[:, None]), g8)


@pytest.mark.parametrize("bits", ["int4", "int8"])
def test_get_quantized_linear(bits, capsys):
    q, fx = armed_quantizer("b", bits)
    with torch.no_grad():
        q.layer.bias = None
    grid, scale, _, _ = q.quantize_weight()
    q2, _ = armed_quantizer("b", bits)
    new = q2.get_quantized_linear(pring_loss=True)
    assert "quant_losses=" in capsys.readouterr().out
    sd = new.state_dict()
    if bits == "int4":
        assert isinstance(new, q4.DynamicQuantizeLinear)
        assert {k: (tuple(v.shape), v.dtype) for k, v in sd.items()} == {"weight": ((160, 64), torch.uint8),
                                                                        "weight_scale": ((10, 64), torch.float32)}
        dense = q4.qlinear.unpack_int4(sd["weight"], sd["weight_scale"]).t()
    else:
        assert isinstance(new, q8.DynamicQuantizeLinear)
        assert {k: (tuple(v.shape), v.dtype) for k, v in sd.items()} == {"weight": ((64, 320), torch.int8),
                                                                        "weight_scale": ((64,), torch.float32)}
        dense = sd["weight"].float() * sd["weight_scale"][:, None]
    assert torch.equal(dense, grid)                              # the module holds exactly the grid weight
    assert torch.equal(sd["weight_scale"], scale)
    x = torch.from_numpy(fx["debug_input"])
    assert torch.allclose(new(x), x @ grid.t(), rtol=1e-4, atol=1e-5)


def test_use_kernel_needs_a_gpu_tensor():
    q, _ = armed_quantizer("a", "int4")
    with pytest.raises(ValueError):
        q.quantize_weight(use_kernel=True)
    with pytest.raises(AssertionError):
        q4.GPTQLinearQuantizer(nn.ReLU())
    fresh = q8.GPTQLinearQuantizer(nn.Linear(32, 8))
    with pytest.raises(AssertionError):
        fresh.quantize_weight()                                  # no calibration input yet


def tiny_float_model(seed=0):
    g = torch.Generator().manual_seed(seed)
    m = ChatGLM2Model(TINY, torch.float32)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, generator=g) * 0.1)
            elif n.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=g) * 0.02)
            else:
                p.fill_(1.0)
    return m.eval()


def tiny_batches(seed=1):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, TINY.vocab_size, (3, 12), generator=g)
    mask = torch.ones(3, 12, dtype=torch.long)
    mask[1, :4] = 0
    return [dict(input_ids=ids, attention_mask=mask), dict(input_ids=torch.randint(0, TINY.vocab_size, (2, 9), generator=g))]


@pytest.mark.parametrize("quant_type", ["int4g32", "int8"])
def test_driver_on_tiny_model(quant_type, tmp_path):
    m = tiny_float_model()
    batches = tiny_batches()
    with torch.no_grad():
        want = m(**batches[0])[1]
    lines = []
    out = gptq_quantize_model_(m, batches, quant_type, log=lines.append)
    assert out is m and len(lines) == 4 * TINY.num_layers + 1 and lines[-1].startswith("lm_head")
    assert not any(isinstance(x, nn.Linear) for x in m.modules())
    twin = (create_quant_int4_model if quant_type == "int4g32" else create_quant_int8_model)(TINY, dtype=torch.float32)
    sig = lambda model: {k: (tuple(v.shape), v.dtype) for k, v in model.state_dict().items()}    # noqa: E731
    assert sig(m) == sig(twin)
    with torch.no_grad():
        got = m(**batches[0])[1]
    rel = float((got - want).norm() / want.norm())
    print(f"{quant_type}: logits of the quantised model against the float model, rel l2 {rel:.4f}")
    # a sanity bound, not a precision claim: logits unrelated to the float model's give sqrt(2); 4-bit weights of a 64-wide
    # model sit near 0.2, 8-bit ones near 0.01 (16 times finer)
    assert rel < (0.5 if quant_type == "int4g32" else 0.05)
    loader.save_model(tmp_path, loader.ChatGLMLoadConfig(model_config=TINY, quant_type=quant_type), m)
    _, back = loader.load_model(tmp_path)
    for k, v in m.state_dict().items():
        assert torch.equal(v, back.state_dict()[k]), k
    with torch.no_grad():
        assert torch.equal(back(**batches[0])[1], got)
    with pytest.raises(ValueError):
        gptq_quantize_model_(tiny_float_model(), batches, "int3")

"""Batched generation, CPU branch: ``ChatGLMDecoder.generate_batch_ids`` (the host form of the per-row step: argmax / the reference's
filtered distribution per row, the same stop rules) against the REFERENCE model's greedy continuation of a left-padded batch
(tests/golden/batch_generate.npz, generator: tests/golden/make_golden_batch_generate.py), and its host-side rules: end token,
per-row budgets, argument errors.  The GPU twin (the HIP kernel, the captured "rows" step) is test_batch_generate_gpu.py."""
import numpy as np
import pytest
import torch

import _golden as G
from chatglm_q_amd import fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build

Z = G.load("batch_generate.npz")


def prompts_of(name):
    ids, attn = Z[f"{name}/ids"], Z[f"{name}/attention_mask"]
    return [ids[b][attn[b] == 1].tolist() for b in range(ids.shape[0])]


@pytest.fixture(scope="module")
def tiny_f32():
    model, cfg = build("f32")
    return model, cfg


def test_fixture_margins_as_recorded():
    """The fixture is what its generator says: margins > 0 everywhere (no exact ties to argue about)."""
    for name, smallest in (("tiny/f32", 0.005), ("tiny/f16", 0.005), ("real/b4", 0.02)):
        mg = Z[f"{name}/margin"]
        assert mg.min() > smallest, (name, mg.min())
        assert Z[f"{name}/tokens"].shape == mg.shape


def test_greedy_batch_equals_reference(tiny_f32):
    """Every one of the 48 (row, step) tokens equals the reference's: the smallest reference margin (0.0055) is thousands of times
    the CPU fp32 noise."""
    model, cfg = tiny_f32
    want = Z["tiny/f32/tokens"]
    dec = ChatGLMDecoder(cfg, model)
    got = dec.generate_batch_ids(prompts_of("tiny/f32"), max_generated_tokens=want.shape[1], greedy=True, ignore_eos=True)
    assert [len(r) for r in got] == [want.shape[1]] * want.shape[0]
    assert np.array_equal(np.array(got), want), (got, want.tolist())
    s = dec.last_stats
    assert s["generated"] == [want.shape[1]] * want.shape[0] and s["steps"] == want.shape[1] - 1


def test_eos_and_budgets(tiny_f32):
    model, cfg = tiny_f32
    prompts = prompts_of("tiny/f32")
    T = 16
    base = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True)
    # an end token that row r produces at step j (its first occurrence), and that no other row produces at all
    pick = None
    for r in range(len(base)):
        for j, t in enumerate(base[r]):
            if 2 <= j < T - 2 and all(t not in base[o] for o in range(len(base)) if o != r):
                pick = (r, base[r].index(t), t)
                break
        if pick:
            break
    assert pick is not None, base
    r, j, eos = pick
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    got = dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True)
    assert got[r] == base[r][:j + 1] and got[r][-1] == eos
    for o in range(len(base)):
        if o != r:
            assert got[o] == base[o]
    # ignore_eos runs through it
    assert dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True) == base
    # per-row budgets cut where they say; budget 0 gives []
    budgets = [5, 0, 11]
    cut = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=budgets, greedy=True, ignore_eos=True)
    assert cut == [base[b][:n] for b, n in enumerate(budgets)]
    assert ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=0, greedy=True) == [[], [], []]
    # the budget is capped by the longest prompt: limit - S
    limit = cfg.max_sequence_length
    S = max(len(p) for p in prompts)
    long = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=10 ** 6, greedy=True, ignore_eos=True)
    assert [len(x) for x in long] == [limit - S] * 3 and [x[:T] for x in long] == base


def test_sampled_rows_on_host(tiny_f32):
    """Sampled rows on the host: repeatable with equal seeds, inside the filtered support, a greedy row among sampled ones is the
    argmax continuation, and the None seed follows torch.manual_seed."""
    model, cfg = tiny_f32
    prompts = prompts_of("tiny/f32")
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=8, ignore_eos=True, top_k=[5, 1, 50], greedy=[False, True, False], temperature=[1.0, 1.0, 0.7])
    a = dec.generate_batch_ids(prompts, seed=[3, 4, 5], **kw)
    b = dec.generate_batch_ids(prompts, seed=[3, 4, 5], **kw)
    assert a == b and [len(x) for x in a] == [8, 8, 8]
    base = dec.generate_batch_ids(prompts, max_generated_tokens=8, greedy=True, ignore_eos=True)
    assert a[1] == base[1]
    torch.manual_seed(123)
    c = dec.generate_batch_ids(prompts, **kw)
    torch.manual_seed(123)
    assert dec.generate_batch_ids(prompts, **kw) == c
    assert all(0 <= t < cfg.vocab_size for row in a + c for t in row)


def test_argument_errors(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], []])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=[4, 4, 4])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], top_k=[4])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], seed=[1, 2, 3])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], temperature=0.0)
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], temperature=[1.0, -1.0])
    with pytest.raises(ValueError):
        dec.generate_batch_ids([[1, 2], [3]], poll_every=0)
    with pytest.raises(RuntimeError):
        dec.generate_batch(["a"])                               # no tokenizer


def test_host_step_rules():
    """The host form of one batched step: finished rows keep their state and get the fill id, a NaN row and an all -inf row give
    an in-range token and the invalid flag, budgets and the stop id finish rows, live counts them."""
    B, N = 5, 40
    rows = fused_ops.BatchRows(B, 6, "cpu")
    rows.arm([(1, 0.8, 1.0)] * B, [1, 2, 3, 4, 5], [3, 1, 4, 0, 4], stop_id=7)
    assert int(rows.live[0]) == 4 and int(rows.row_state[3, 1]) == fused_ops.BatchRows.FINISHED
    x = torch.randn(B, N, generator=torch.Generator().manual_seed(1))
    x[0, 7] = 50.0                                              # row 0 hits the stop id
    x[2] = float("nan")
    x[4] = float("-inf")
    tok = torch.zeros(B, dtype=torch.int64)
    fused_ops.batch_sample_advance(x, tok, rows)
    st = rows.row_state
    assert tok[0] == 7 and st[0].tolist() == [1, 1]
    assert tok[1] == int(x[1].argmax()) and st[1].tolist() == [1, 1]      # budget 1
    assert tok[2] == 0 and st[2].tolist() == [1, 3]                       # all NaN: 0, finished + invalid
    assert tok[3] == 7 and st[3].tolist() == [0, 1]                       # armed finished: the fill id, nothing recorded
    assert tok[4] == 0 and st[4].tolist() == [1, 3]                       # all -inf
    assert int(rows.live[0]) == 0
    before = (rows.row_state.clone(), rows.row_rng.clone(), rows.out_tokens.clone())
    fused_ops.batch_sample_advance(x, tok, rows)
    assert torch.equal(rows.row_state, before[0]) and torch.equal(rows.row_rng, before[1]) and torch.equal(rows.out_tokens, before[2])
    assert tok.tolist() == [7] * B
    with pytest.raises(ValueError):
        rows.arm([(1, 0.8, 0.0)] * B, [1] * B, [1] * B)
    with pytest.raises(ValueError):
        rows.arm([(1, 0.8, 1.0)] * (B - 1), [1] * B, [1] * B)

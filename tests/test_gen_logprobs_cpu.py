"""Log-probabilities during generation, CPU branch: the host form of ``fused_ops.step_logprobs`` against the float64 oracle
(tests/_logprobs_oracle.py), its skip and full rules, ``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` with ``logprobs=``
against a teacher-forced eager loop written there, and the ABI.  The GPU twin (the HIP kernel, the captured "+lp" steps) is
test_gen_logprobs_gpu.py."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _logprobs_oracle as LO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, GenerationLogprobs
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 4.0            # tests/test_score_gpu.py: the bar against float64 is FACTOR x the error of torch's CPU fp32 F.cross_entropy
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NINF = float("-inf")


def make_rows(B, N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, generator=g) * torch.tensor([1.0, 4.0, 12.0]).repeat(-(-B // 3))[:B, None]
    if N >= 7:
        x[0, 3] = x[0, 5] = x[0].max() + 1                       # a tie at the top: the lower index first
        x[1, N - 1] = NINF
    return x.to(dtype)


@pytest.mark.parametrize("n_top", [0, 1, 5, 20])
@pytest.mark.parametrize("N", [1, 7, 1000])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_host_form_against_the_oracle(dt, N, n_top):
    B = 3
    x = make_rows(B, N, TDT[dt], 100 * N + n_top)
    tok = torch.tensor([0, N - 1, N // 2], dtype=torch.int64)
    st = fused_ops.StepLogprobs(B, 4, "cpu", n_top=n_top)
    st.count.copy_(torch.tensor([0, 1, 3], dtype=torch.int32))
    fused_ops.step_logprobs(x, tok, st)
    assert st.count.tolist() == [1, 2, 4]
    x64 = x.double().numpy()
    lsm64 = LO.log_softmax64(x64)
    # the reference's own arithmetic on the same rows against float64: F.cross_entropy at every id of every row
    ref = -F.cross_entropy(x.float().repeat_interleave(N, dim=0), torch.arange(N).repeat(B), reduction="none").view(B, N).numpy()
    e_ref = LO.metric(ref, lsm64)
    got_c, want_c, got_t, want_t = [], [], [], []
    for b, c in enumerate([0, 1, 3]):
        got_c.append(float(st.chosen[b, c]))
        want_c.append(lsm64[b, int(tok[b])])
        if n_top:
            ids, lp = LO.top(x64[b], n_top)
            assert st.top_ids[b, c].tolist() == ids.tolist(), (dt, N, n_top, b)
            got_t.append(st.top_lp[b, c].numpy())
            want_t.append(lp)
            if N < n_top:
                assert st.top_ids[b, c, N:].tolist() == [-1] * (n_top - N) and bool((st.top_lp[b, c, N:] == NINF).all())
    e = LO.metric(got_c, want_c)
    e_top = LO.metric(np.stack(got_t), np.stack(want_t)) if n_top else 0.0
    print(f"[step_logprobs host] {dt} N={N} n_top={n_top}: chosen err {e:.3e}, alternatives err {e_top:.3e} (fp32 cross_entropy: {e_ref:.3e})")
    assert e <= FACTOR * e_ref and e_top <= FACTOR * e_ref


def test_skip_rule_and_full_rule():
    B, N, cap = 4, 50, 3
    x = torch.randn(B, N, generator=torch.Generator().manual_seed(1))
    tok = torch.tensor([1, 2, 3, 4], dtype=torch.int64)
    st = fused_ops.StepLogprobs(B, cap, "cpu", n_top=2)
    for t in st.tensors()[1:]:
        t.fill_(-7)
    st.count.copy_(torch.tensor([0, 2, 1, 3], dtype=torch.int32))
    # row 0: live (1 token, 0 recorded); row 1: finished (2 tokens, 2 recorded); row 2: live (2 > 1); row 3: live but the record is full
    row_state = torch.tensor([[1, 0], [2, 1], [2, 0], [4, 0]], dtype=torch.int32)
    before = [t.clone() for t in st.tensors()]
    fused_ops.step_logprobs(x, tok, st, row_state)
    assert st.count.tolist() == [1, 2, 2, 3]
    lsm = torch.log_softmax(x, dim=-1)
    assert float(st.chosen[0, 0]) == float(lsm[0, 1]) and float(st.chosen[2, 1]) == float(lsm[2, 3])
    assert st.top_ids[0, 0].tolist() == LO.order(x[0].numpy())[:2].tolist()
    for b, c in ((0, 0), (2, 1)):                                # nothing but the slot written moved
        for t in before[1:]:
            t[b, c] = -7
    for t in st.tensors()[1:]:
        t[0, 0] = -7
        t[2, 1] = -7
    assert all(torch.equal(a, b_) for a, b_ in zip(before[1:], st.tensors()[1:]))
    # without a row_state every row records, except the full one
    fused_ops.step_logprobs(x, tok, st)
    assert st.count.tolist() == [2, 3, 3, 3]
    # a chosen id outside the vocabulary: NaN; arm() forgets the record
    st.arm()
    assert st.count.tolist() == [0] * B
    fused_ops.step_logprobs(x, torch.tensor([N, -1, 0, 0], dtype=torch.int64), st)
    assert np.isnan(st.read(0)[0][0]) and np.isnan(st.read(1)[0][0]) and st.read(2)[0] == [float(lsm[2, 0])]
    assert st.read(2, 1, limit=5)[1] == [[int(LO.order(x[2].numpy())[0])]] and st.read(2, 0, limit=0) == ([], [], [])
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(x[:2], tok[:2], st)
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(x, tok.int(), st)
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(x, tok, st, row_state.long())
    with pytest.raises(ValueError):
        fused_ops.StepLogprobs(1, 4, "cpu", n_top=fused_ops.TOP_LOGPROBS_MAX + 1)


@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


def test_generate_ids_greedy_logprobs_equal_the_loop(tiny_f32):
    model, cfg = tiny_f32
    p = [17, 3, 99, 250, 8, 61]
    T = 12
    dec = ChatGLMDecoder(cfg, model)
    base = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    assert dec.last_logprobs is None and dec.last_stats["logprobs"] is False
    got = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, logprobs=3))
    rec = dec.last_logprobs
    assert got == base and dec.last_stats["logprobs"] is True and isinstance(rec, GenerationLogprobs)
    assert len(rec.token_logprobs) == len(got) == T
    assert all(rec.top_ids[t][0] == got[t] and len(rec.top_ids[t]) == 3 for t in range(T))
    assert all(rec.top_logprobs[t][0] == rec.token_logprobs[t] for t in range(T))
    LO.check_record(LO.replay_logits(model, [p], [got]), [got], [rec], 3)
    # sampled on the host (the CPU's only sampler), with penalties: the record is that of the adjusted logits
    kw = dict(repetition_penalty=1.3, presence_penalty=0.4, logit_bias={base[0]: NINF})
    torch.manual_seed(5)
    plain = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, **kw))
    torch.manual_seed(5)
    got = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, logprobs=0, **kw))
    assert got == plain and dec.last_logprobs.top_ids == [[]] * T
    LO.check_record(LO.replay_logits(model, [p], [got], [(1.3, 0.4, 0.0)], [kw["logit_bias"]]), [got], [dec.last_logprobs], 0)
    # a generator closed early: the record holds the tokens handed out
    gen = dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, logprobs=1)
    first = [next(gen), next(gen), next(gen)]
    gen.close()
    assert first == base[:3] and dec.last_logprobs.token_logprobs == rec.token_logprobs[:3]


def test_generate_batch_ids_logprobs_equal_the_loop(tiny_f32):
    model, cfg = tiny_f32
    prompts = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0]]
    budgets = [10, 2, 10]
    r, p, f = [1.5, 1.0, 1.2], [0.0, 0.7, 0.0], [0.4, 0.0, 0.1]
    dec = ChatGLMDecoder(cfg, model)
    first = dec.generate_batch_ids(prompts, max_generated_tokens=budgets, greedy=True, ignore_eos=True)
    bias = [None, {first[1][0]: -1.0}, {first[2][0]: NINF}]
    kw = dict(max_generated_tokens=budgets, greedy=True, ignore_eos=True, repetition_penalty=r, presence_penalty=p,
              frequency_penalty=f, logit_bias=bias)
    base = dec.generate_batch_ids(prompts, **kw)
    assert dec.last_logprobs is None and dec.last_stats["logprobs"] is False
    got = dec.generate_batch_ids(prompts, logprobs=3, **kw)
    recs = dec.last_logprobs
    assert got == base and [len(g) for g in got] == budgets and dec.last_stats["logprobs"] is True
    assert [len(rc.token_logprobs) for rc in recs] == budgets
    assert all(rc.top_ids[t][0] == g[t] for rc, g in zip(recs, got) for t in range(len(g)))
    LO.check_record(LO.replay_logits(model, prompts, got, list(zip(r, p, f)), bias), got, recs, 3)
    # a row with budget 0 records nothing
    dec.generate_batch_ids(prompts, max_generated_tokens=[3, 0, 1], greedy=True, ignore_eos=True, logprobs=2)
    assert [len(rc.token_logprobs) for rc in dec.last_logprobs] == [3, 0, 1]


def test_logprobs_argument(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    assert dec.last_logprobs is None
    list(dec.generate_ids([1, 2, 3], max_generated_tokens=3, greedy=True, logprobs=None))
    assert dec.last_logprobs is None and dec.last_stats["logprobs"] is False
    assert dec._session.lp is None                              # never asked for: nothing allocated
    for bad in (21, -1, True, 2.0, "3"):
        with pytest.raises(ValueError):
            list(dec.generate_ids([1, 2, 3], max_generated_tokens=3, greedy=True, logprobs=bad))
        with pytest.raises(ValueError):
            dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=3, greedy=True, logprobs=bad)
    list(dec.generate_ids([1, 2, 3], max_generated_tokens=3, greedy=True, ignore_eos=True, logprobs=20))
    assert [len(t) for t in dec.last_logprobs.top_ids] == [20] * 3
    list(dec.generate_ids([1, 2, 3], max_generated_tokens=3, greedy=True, ignore_eos=True))
    assert dec.last_logprobs is None
    assert list(dec.generate_ids([1, 2, 3], max_generated_tokens=0, greedy=True, logprobs=2)) == [] and len(dec.last_logprobs) == 0
    assert dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=0, greedy=True, logprobs=2) == [[], []]
    assert [len(r) for r in dec.last_logprobs] == [0, 0]


def test_abi_declares_and_exports_the_entry_point():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"\bint\s+qlinear_step_logprobs\s*\(", header)
    assert re.search(r"#define\s+QL_TOP_LOGPROBS_MAX\s+20\b", header)
    assert re.search(r"#define\s+QLINEAR_ABI_VERSION\s+3\b", header)
    assert "qlinear_step_logprobs" in _lib.EXPORTS and fused_ops.TOP_LOGPROBS_MAX == 20
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), "qlinear_step_logprobs") is not None
    assert getattr(ctypes.CDLL(_lib.DEV_LIB_PATH), "qlinear_step_logprobs") is not None

"""Beam search on the CPU: the Python oracle (tests/_beam_oracle.py) against an exhaustive enumeration, the host forms of
``fused_ops.beam_advance`` / ``beam_gather`` against the oracle, and ``ChatGLMDecoder.beam_search_ids`` on the tiny model."""
import itertools
import os
import re

import numpy as np
import pytest
import torch

import _beam_cases as BC
import _beam_oracle as BO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import BeamHypothesis, ChatGLMDecoder, DecodeSession
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


# ---- the oracle is meaningful -----------------------------------------------------------------------------------------------------
def markov_logprobs(seed):
    """A first-order Markov "model" over ids 0..3 plus the end id 4: row ``last`` of a fixed random logit table -> fp32 log-probs."""
    rng = np.random.default_rng(seed)
    table = rng.normal(size=(5, 5)).astype(np.float32) * F(2)
    out = []
    for row in table:
        m = row.max()
        ls = np.log(np.exp(row - m, dtype=np.float32).sum(dtype=np.float32), dtype=np.float32)
        out.append(((row - m) - ls).astype(np.float32))
    return out


def row_candidates(lp_row):
    order = sorted(range(5), key=lambda i: (-float(lp_row[i]), i))
    return order, [lp_row[i] for i in order]


@pytest.mark.parametrize("seed", range(8))
def test_oracle_finds_what_exhaustive_enumeration_ranks_first(seed):
    END, T, B, START = 4, 3, 16, 0                               # 16 = the distinct 2-token prefixes without the end id
    lp = markov_logprobs(seed)
    # every sequence that ends on END within T tokens, and every T-token sequence without it: the sum in generation order
    best = None
    for n in range(1, T + 1):
        for body in itertools.product(range(4), repeat=n - 1):
            tails = [(END,)] if n < T else [(i,) for i in range(5)]
            for tail in tails:
                seq, total, last = body + tail, F(0), START
                for i in seq:
                    total = BO.fadd(total, lp[last][i])
                    last = i
                if best is None or float(total) > float(best[1]):
                    best = (list(seq), total)
    # length_penalty 0: the score is the sum.  early_stopping=False: a search only ends when no running beam can beat the heap
    beams = BO.Beams(1, B, END, 0.0, False, T)
    last = [START] * B
    for _ in range(T):
        cands = [row_candidates(lp[last[r]]) for r in range(B)]
        last, _ = beams.advance([c[0] for c in cands], [c[1] for c in cands])
    ids, score, total = beams.finalize(1)[0][0]
    assert ids == best[0]
    assert np.float32(total).view(np.int32) == np.float32(best[1]).view(np.int32) and float(score) == float(total)


# ---- the host forms against the oracle --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,B", [(1, 1), (1, 2), (3, 4), (1, 10), (3, 2)])
@pytest.mark.parametrize("length_penalty,early", [(0.0, False), (1.0, True), (2.5, False)])
def test_host_advance_equals_oracle(P, B, length_penalty, early):
    events = {}
    for seed in range(3):
        o = BC.run_scenario("cpu", P, B, 11, length_penalty, early, n_steps=10, cap=9, seed=seed, book=seed == 1)
        for k, v in o.events.items():
            events[k] = events.get(k, 0) + v
    assert events.get("heap_append", 0) > 0 and events.get("ride_full", 0) + events.get("ride_done", 0) > 0


def test_scenarios_cover_the_named_cases():
    """What the GPU test relies on as well: the shared scenarios meet every case of the rules."""
    events = {}
    for P, B, lp, early in BC.CONFIGS:
        for seed in range(3):
            o = BC.run_scenario("cpu", P, B, 11, lp, early, n_steps=10, cap=9, seed=seed)
            for k, v in o.events.items():
                events[k] = events.get(k, 0) + v
    for k in ("heap_append", "heap_replace", "heap_keep_equal", "heap_keep_less", "end_skipped", "tie_across_rows", "done", "ride_done",
              "ride_full"):
        assert events.get(k, 0) > 0, (k, events)


def test_no_end_token_never_finishes():
    o = BC.run_scenario("cpu", 2, 3, None, 1.0, True, n_steps=5, cap=8, seed=0)
    assert o.live == 2 and o.heap == [[], []]
    hyps = o.finalize(2)
    assert all(len(h) == 2 and len(h[0][0]) == 5 for h in hyps)


@pytest.mark.parametrize("kind", ["identity", "first", "cycle", "dup", "outside"])
def test_host_gather_equals_index_select(kind):
    for B, P in ((2, 1), (4, 2), (10, 1)):
        BC.run_gather("cpu", P, B, 16, (2, 3), torch.float16, kind, 3, 9)
        BC.run_gather("cpu", P, B, 16, (4,), torch.float32, kind, 0, 16)
        BC.run_gather("cpu", P, B, 16, (4,), torch.float32, kind, 8, 9)
        BC.run_gather("cpu", P, B, 16, (4,), torch.float32, kind, 9, 9)


def test_argument_errors():
    st = fused_ops.BeamState(4, 8, "cpu")
    tok = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError):
        fused_ops.beam_advance(st, tok)                          # not armed
    for P, B in ((1, 0), (1, 11), (3, 1), (1, 3)):
        with pytest.raises(ValueError):
            st.arm(P, B)
    with pytest.raises(ValueError):
        st.arm(2, 2, length_penalty=float("nan"))
    st.arm(2, 2)
    with pytest.raises(ValueError):
        fused_ops.beam_advance(st, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        fused_ops.beam_advance(st, tok, write_index=torch.zeros(1, dtype=torch.int64))       # pos and mask are missing
    bufs = [torch.zeros(4, 8, 2, 4)]
    table = fused_ops.BeamGatherTable(bufs)
    first, end = torch.zeros(1, dtype=torch.int32), torch.ones(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        fused_ops.beam_gather(table, torch.zeros(4, dtype=torch.int64), first, end, 2)       # parent must be int32
    with pytest.raises(ValueError):
        fused_ops.beam_gather(table, torch.zeros(4, dtype=torch.int32), first, end, 3)       # 3 does not divide 4 rows
    with pytest.raises(ValueError):
        fused_ops.BeamGatherTable([torch.zeros(4, 8, 2), torch.zeros(4, 8, 3)])
    with pytest.raises(ValueError):
        fused_ops.BeamGatherTable([torch.zeros(4, 8, 2, 4).transpose(0, 1)])


def test_declarations():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"^int qlinear_beam_advance\(", header, re.M) and re.search(r"^int qlinear_beam_gather\(", header, re.M)
    assert re.search(r"^#define QL_BEAMS_MAX 10$", header, re.M) and fused_ops.BEAMS_MAX == 10
    assert 2 * fused_ops.BEAMS_MAX <= fused_ops.TOP_LOGPROBS_MAX
    assert re.search(r"^#define QLINEAR_ABI_VERSION 3$", header, re.M) and "Still 3: qlinear_beam_advance and qlinear_beam_gather" in header
    assert "qlinear_beam_advance" in _lib.EXPORTS and "qlinear_beam_gather" in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, "chatglm_q_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "beam_search.hip" in srcs and os.path.exists(os.path.join(ROOT, "chatglm_q_amd", "csrc", "beam_search.hip"))


# ---- the tiny model ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


PROMPT, T = [17, 3, 99, 250, 8, 61], 10


def test_one_beam_is_greedy(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    greedy = list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True, ignore_eos=True))
    hyps = dec.beam_search_ids(PROMPT, num_beams=1, max_generated_tokens=T, ignore_eos=True)
    assert len(hyps) == 1 and isinstance(hyps[0], BeamHypothesis) and hyps[0].ids == greedy
    eos = greedy[3]
    assert eos not in greedy[:3]
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    assert dec.beam_search_ids([PROMPT], num_beams=1, max_generated_tokens=T)[0][0].ids == greedy[:4]
    assert list(dec.generate_ids(PROMPT, max_generated_tokens=T, greedy=True)) == greedy[:4]


def test_scores_sorted_and_num_return_sequences(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    prompts = [PROMPT, [44, 3]]
    out = dec.beam_search_ids(prompts, num_beams=4, max_generated_tokens=T, num_return_sequences=3, ignore_eos=True)
    assert len(out) == 2 and all(len(h) == 3 for h in out)
    for hyps in out:
        scores = [h.score for h in hyps]
        assert scores == sorted(scores, reverse=True) and all(len(h.ids) == T for h in hyps)
        assert all(abs(h.score - h.sum_logprob / T) < 1e-5 for h in hyps)                    # length_penalty 1
        assert len({tuple(h.ids) for h in hyps}) == 3
    assert len(dec.beam_search_ids(prompts, num_beams=4, max_generated_tokens=T, ignore_eos=True)[1]) == 1
    s = dec.last_stats
    assert s["beams"] == 4 and s["prompts"] == 2 and s["steps"] == T - 1 and s["prefill_s"] > 0 and s["steps_per_s"] > 0
    # the best of 4 beams is at least as likely as the greedy sequence (greedy is beam 0's path while nothing beats it)
    one = dec.beam_search_ids(PROMPT, num_beams=1, max_generated_tokens=T, ignore_eos=True, length_penalty=0.0)[0]
    four = dec.beam_search_ids(PROMPT, num_beams=4, max_generated_tokens=T, ignore_eos=True, length_penalty=0.0)[0]
    assert four.sum_logprob >= one.sum_logprob
    # a batch row's result does not depend on its neighbours
    solo = dec.beam_search_ids([PROMPT], num_beams=4, max_generated_tokens=T, num_return_sequences=3, ignore_eos=True)[0]
    assert [h.ids for h in solo] == [h.ids for h in out[0]]
    # a budget of 0
    assert dec.beam_search_ids(prompts, num_beams=2, max_generated_tokens=0) == [[], []]


def test_end_token_finishes_hypotheses(tiny_f32):
    model, cfg = tiny_f32
    base = ChatGLMDecoder(cfg, model).beam_search_ids(PROMPT, num_beams=3, max_generated_tokens=T, ignore_eos=True)[0].ids
    eos = base[2]
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    for early in (True, False):
        hyps = dec.beam_search_ids(PROMPT, num_beams=3, max_generated_tokens=T, early_stopping=early, num_return_sequences=3)
        assert any(h.ids[-1] == eos for h in hyps)
        assert all(eos not in h.ids[:-1] for h in hyps)
        assert [h.score for h in hyps] == sorted((h.score for h in hyps), reverse=True)


def test_api_argument_errors(tiny_f32, monkeypatch):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    for kw in (dict(num_beams=0), dict(num_beams=11), dict(num_beams=2, num_return_sequences=3), dict(num_return_sequences=0),
               dict(num_beams=2.0), dict(length_penalty=float("inf")), dict(poll_every=0)):
        with pytest.raises(ValueError):
            dec.beam_search_ids(PROMPT, max_generated_tokens=4, **kw)
    for prompts in ([], [[]], [PROMPT, []]):
        with pytest.raises(ValueError):
            dec.beam_search_ids(prompts, max_generated_tokens=4)
    monkeypatch.setattr(model.config, "vocab_size", 7)
    with pytest.raises(ValueError):
        dec.beam_search_ids(PROMPT, num_beams=4, max_generated_tokens=4)
    with pytest.raises(ValueError):
        DecodeSession(model, 4, 16, use_graph=False).arm_beams(4)

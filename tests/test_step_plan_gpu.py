"""The decode step's plan on the GPU: with every stage on, the eager steps of the device's three selectors launch the stages in order, then
the selection - ``greedy_advance``, ``top_p_sample`` or ``batch_sample_advance`` - then the record (the recorder of test_step_plan_cpu)."""
import pytest

import test_pda_gpu as TPG
import test_step_plan_cpu as TSC
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build as build_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T = TSC.T


@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


@pytest.mark.parametrize("grammar", ["dfa", "pda"])
def test_selection_sits_between_the_stages_and_the_record(tiny16, monkeypatch, grammar):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model, eos_token_id=TPG.tiny_vocab(cfg.vocab_size)[1], token_bytes=TPG.TOKEN_BYTES())
    calls = TSC.record_launches(monkeypatch)
    kw = dict(TSC.controls(True, True, grammar, 2), use_graph=False)
    stages_then = lambda selection: TSC.one_token(True, True, grammar, 2, selection)
    assert stages_then("x")[-2:] == ["x", "step_logprobs"] and len(stages_then("x")) == 5

    # device greedy: the first token's argmax is a torch op behind the prefill, every step's is the launch
    ids = list(dec.generate_ids(TPG.P1, greedy=True, **kw))
    assert 1 <= len(ids) <= T and calls == stages_then(None) + stages_then("greedy_advance") * (len(ids) - 1), calls
    # the device sampler
    del calls[:]
    ids = list(dec.generate_ids(TPG.P1, seed=5, **kw))
    assert 1 <= len(ids) <= T and calls == stages_then("top_p_sample") * len(ids), calls
    # rows: batch 1 and batch 3
    for prompts in ([TPG.P1], TPG.PROMPTS[:3]):
        del calls[:]
        out = dec.generate_batch_ids(prompts, seed=7, **kw)
        tokens = 1 + dec.last_stats["steps"]
        assert max(len(o) for o in out) <= tokens <= T and calls == stages_then("batch_sample_advance") * tokens, calls

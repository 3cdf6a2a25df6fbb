"""The decode step's plan: the order of the launches of one step over the whole feature matrix - penalties x history constraints x
grammar {none, DFA, pushdown} x log-prob record, through ``generate_ids`` (greedy and host-sampled) and ``generate_batch_ids`` - with a
recorder around every ``fused_ops`` entry of a step, and the graph key of all 512 flag combinations against the rule written out here."""
import itertools

import pytest
import torch

import test_grammar_cpu as TG
import test_pda_cpu as TPC
from chatglm_q_amd import decoder as D
from chatglm_q_amd import fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build

STAGES = ("logit_penalties", "history_constraints", "grammar_mask", "pda_mask")
SELECTIONS = ("greedy_advance", "top_p_sample", "batch_sample_advance")
RECORDED = STAGES + SELECTIONS + ("step_logprobs",)
T = 4                                                           # tokens per generation
GRAMMARS = {"none": None, "dfa": "[A-D]+", "pda": TPC.J(True, max_depth=4)}
MATRIX = list(itertools.product((False, True), (False, True), GRAMMARS, (None, 2)))


def record_launches(monkeypatch):
    """Every ``fused_ops`` entry of a step wrapped so that a call appends its name to the returned list (the decoder looks them up
    through the module at call time)."""
    calls = []
    for name in RECORDED:
        def wrapped(*args, _real=getattr(fused_ops, name), _name=name, **kw):
            calls.append(_name)
            return _real(*args, **kw)
        monkeypatch.setattr(fused_ops, name, wrapped)
    return calls


def controls(pen, con, grammar, logprobs):
    kw = dict(max_generated_tokens=T, logprobs=logprobs)
    if pen:
        kw.update(repetition_penalty=1.3, frequency_penalty=0.2)
    if con:
        kw.update(no_repeat_ngram_size=2)
    if GRAMMARS[grammar] is not None:
        kw.update(grammar=GRAMMARS[grammar])
    return kw


def one_token(pen, con, grammar, logprobs, selection=None):
    """The launches of one token: [pen][con][gr|pda] [the selection's, when a launch makes it] [the record's]."""
    stage = [s for s, on in zip(STAGES, (pen, con, grammar == "dfa", grammar == "pda")) if on]
    return stage + ([selection] if selection else []) + (["step_logprobs"] if logprobs is not None else [])


@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


def test_launch_order_over_the_matrix(tiny_f32, monkeypatch):
    model, cfg = tiny_f32
    vocab, eos = TPC.tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=vocab)
    calls = record_launches(monkeypatch)
    torch.manual_seed(0)
    for pen, con, grammar, logprobs in MATRIX:
        kw = controls(pen, con, grammar, logprobs)
        case = (pen, con, grammar, logprobs)
        # on the CPU the argmax and the reference's sampler are torch ops on the host's side: no selection launch
        for mode in (dict(greedy=True), dict(device_sampler=False)):
            del calls[:]
            ids = list(dec.generate_ids(TG.PROMPT, **kw, **mode))
            assert 1 <= len(ids) <= T and calls == one_token(*case) * len(ids), (case, mode, calls)
        del calls[:]
        out = dec.generate_batch_ids(TG.PROMPTS, greedy=True, **kw)
        tokens = 1 + dec.last_stats["steps"]                     # the first token and every step run (finished rows ride along)
        assert max(len(o) for o in out) <= tokens <= T and calls == one_token(*case, "batch_sample_advance") * tokens, (case, calls)


def expected_key(greedy, sample, rows, pen, lp, con, beam, gr, pda):
    """The rule of the graph keys: "beam" and "logits" bare; otherwise the selector - rows over sample over greedy - and one suffix per
    launch in launch order, the record's last."""
    if beam:
        return "beam"
    selector = "rows" if rows else "sample" if sample else "greedy" if greedy else "logits"
    if selector == "logits":
        return selector
    return selector + "".join("+" + tag for tag, on in (("pen", pen), ("con", con), ("gr", gr), ("pda", pda), ("lp", lp)) if on)


FLAGS = ("greedy", "sample", "rows", "pen", "lp", "con", "beam", "gr", "pda")


def test_graph_keys_of_all_flag_combinations():
    assert [expected_key(*(n in on for n in FLAGS)) for on in (("greedy",), (), ("beam", "pen"), ("sample", "pen"),
                                                               ("rows", "sample", "greedy", "pen", "con", "gr", "lp"))] \
        == ["greedy", "logits", "beam", "sample+pen", "rows+pen+con+gr+lp"]
    seen = set()
    for values in itertools.product((False, True), repeat=len(FLAGS)):
        flags = dict(zip(FLAGS, values))
        plan = D.step_plan(**flags)
        key = expected_key(**flags)
        seen.add(key)
        assert plan.key == key, flags
        assert D.step_plan(**flags) is plan and D.step_plan(*values) is plan          # memoised: a replayed step costs one lookup
        # the plan says what the key says; a "logits" step launches nothing itself: its plan keeps what the caller applies afterwards
        in_step = plan.selector != "logits"
        assert plan.selector == key.split("+")[0] and (plan.lp and in_step) == key.endswith("+lp")
        assert list(plan.in_step) == [t for t in key.split("+")[1:] if t != "lp"]
        asked = [] if flags["beam"] else [tag for tag, _, _, _ in D.LOGIT_STAGES if flags[tag]]
        assert list(plan.stages) == asked and plan.lp == (flags["lp"] and not flags["beam"]) and (not in_step or plan.in_step == plan.stages)
    assert len(seen) == 2 + 3 * 32

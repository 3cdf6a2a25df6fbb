"""Sampling controls, CPU branch: the host form of ``fused_ops.logit_penalties`` against the numpy oracle (tests/_penalty_oracle.py)
bit for bit, ``PenaltyState``'s validation, and ``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` with penalties and a logit
bias against a loop written here (prefill, eager step logits, the oracle, argmax).  The GPU twin (the HIP kernel, the captured
"+pen" steps) is test_penalties_gpu.py."""
import numpy as np
import pytest
import torch

import _penalty_oracle as PO
from chatglm_q_amd import fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build

NINF = float("-inf")


def random_logits(B, N, dt, seed):
    """Normal logits with a few exact zeros, negative zeros, infinities and NaNs sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, N, generator=g) * 4
    flat = x.view(-1)
    idx = torch.randperm(B * N, generator=g)[:min(10, B * N)]
    special = [0.0, -0.0, float("inf"), NINF, float("nan"), 1e-30, -1e-30, 65504.0, -7.0, 3.0]
    for i, v in zip(idx.tolist(), special):
        flat[i] = v
    return x.to(PO.DTYPES[dt])


@pytest.mark.parametrize("N", [7, 64, 1000])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_host_form_equals_oracle(dt, N):
    B, steps = 3, 6
    g = torch.Generator().manual_seed(N)
    prompts = [torch.randint(0, N, (5,), generator=g).tolist(), [], torch.randint(0, N, (12,), generator=g).tolist()]
    settings = [(1.3, 0.5, 0.25), (0.7, -0.4, 0.1), (1.0, 0.0, 0.0)]
    biases = [{1: -3.5, N - 1: NINF}, None, {0: 2.0, 3: NINF, 5: -0.125}]
    st = fused_ops.PenaltyState(B, N, "cpu").arm(prompts, settings, biases)
    assert st.active
    hist = [PO.History(p, N) for p in prompts]
    tok = None
    for s in range(steps):
        x = random_logits(B, N, dt, 100 * N + s)
        want = PO.to_native(x)
        if tok is not None:
            for b in range(B):
                hist[b].count(int(tok[b]))
        for b in range(B):
            want[b] = PO.penalize(want[b], dt, hist[b].P, hist[b].G, *settings[b], bias=biases[b])
        out = fused_ops.logit_penalties(x, st, tok)
        assert out is x
        ok = PO.same(PO.to_native(x), want, dt)
        assert ok.all(), (dt, N, s, np.argwhere(~ok)[:5])
        # the next step's tokens: duplicates on purpose (token 2 again and again in row 0, the prompt's first id in row 2)
        tok = torch.tensor([2, int(torch.randint(0, N, (1,), generator=g)), prompts[2][0]], dtype=torch.int64)
    assert st.generated()[0, 2] == steps - 1 and st.generated().sum(dim=1).tolist() == [steps - 1] * B


def test_counts_advance_only_through_tok_and_finished_rows_are_untouched():
    B, N = 3, 50
    st = fused_ops.PenaltyState(B, N, "cpu").arm([[1, 2], [3], [4]], [(2.0, 1.0, 1.0)] * B, [{7: 1.0}] * B)
    x0 = torch.randn(B, N, generator=torch.Generator().manual_seed(3))
    x = x0.clone()
    fused_ops.logit_penalties(x, st, None)                       # the first token after a prefill: nothing is counted
    assert int(st.generated().sum()) == 0
    assert not torch.equal(x[0], x0[0])
    row_state = torch.zeros((B, 2), dtype=torch.int32)
    row_state[1, 1] = fused_ops.BatchRows.FINISHED
    x = x0.clone()
    fused_ops.logit_penalties(x, st, torch.tensor([9, 9, 9]), row_state)
    assert st.generated()[:, 9].tolist() == [1, 0, 1] and int(st.generated().sum()) == 2
    assert torch.equal(x[1], x0[1]) and not torch.equal(x[0], x0[0]) and not torch.equal(x[2], x0[2])
    # an entry no rule touches keeps its bits; a touched one follows the rules
    want = PO.penalize(x0[0].numpy(), "f32", PO.History([1, 2], N).count(9).P, PO.History([1, 2], N).count(9).G, 2.0, 1.0, 1.0, {7: 1.0})
    assert np.array_equal(x[0].numpy(), want)
    untouched = [v for v in range(N) if v not in (1, 2, 7, 9)]
    assert torch.equal(x[0, untouched], x0[0, untouched])
    # re-arming forgets the history
    st.arm([[1], [1], [1]], [(2.0, 0.0, 0.0)] * B, None)
    assert int(st.generated().sum()) == 0 and int((st.counts != 0).sum()) == B


def test_state_validation():
    N = 100
    st = fused_ops.PenaltyState(2, N, "cpu")
    ok = [(1.1, 0.0, 0.0), (1.0, 0.2, 0.3)]

    def bad(settings=ok, biases=None, prompts=([1], [2]), match=None):
        with pytest.raises(ValueError, match=match):
            st.arm(list(prompts), settings, biases)

    bad(settings=[(1.1, 0, 0), (0.0, 0, 0)], match="row 1")
    bad(settings=[(-1.0, 0, 0), (1.0, 0, 0)], match="row 0")
    bad(settings=[(float("nan"), 0, 0), (1.0, 0, 0)], match="row 0")
    bad(settings=[(float("inf"), 0, 0), (1.0, 0, 0)], match="row 0")
    bad(settings=[(1.0, 0, 0), (1.0, float("nan"), 0)], match="row 1")
    bad(settings=[(1.0, 0, 0), (1.0, 0, float("nan"))], match="row 1")
    bad(settings=[(1.0, float("inf"), 0), (1.0, 0, 0)], match="row 0")
    bad(biases=[None, {3: float("inf")}], match="row 1")
    bad(biases=[{3: float("nan")}, None], match="row 0")
    bad(biases=[None, {N: 1.0}], match="row 1")
    bad(biases=[None, {-1: 1.0}], match="row 1")
    bad(biases=[None, [(3, 1.0), (3, 2.0)]], match="row 1")      # a duplicate id (a dict cannot hold one: the pair form)
    bad(biases=[{i: 0.5 for i in range(fused_ops.LOGIT_BIAS_MAX + 1)}, None], match="row 0")
    bad(settings=ok[:1])
    bad(biases=[None])
    bad(prompts=([1],))
    bad(prompts=([1], [N]), match="row 1")
    assert fused_ops.LOGIT_BIAS_MAX >= 32
    st.arm([[1], [2]], ok, [{i: NINF for i in range(fused_ops.LOGIT_BIAS_MAX)}, None])   # the cap itself, -inf values: fine
    assert st.active
    assert not st.arm([[1], [2]], [(1.0, 0.0, 0.0)] * 2, [None, {}]).active
    with pytest.raises(ValueError):
        fused_ops.logit_penalties(torch.zeros(2, N + 1), st)
    with pytest.raises(ValueError):
        fused_ops.logit_penalties(torch.zeros(2, N), st, torch.zeros(3, dtype=torch.int64))


@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


def loop_tokens(model, prompts, T, settings, biases, pad_id=0):
    """The test's own loop: prefill the left-padded batch, read the eager step logits, apply the oracle per row, take the argmax
    (lowest index on ties), feed it back."""
    B, S, N = len(prompts), max(len(p) for p in prompts), model.config.vocab_size
    ids = torch.full((B, S), pad_id, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    dev = model.final_ln.weight.device
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    dt = {torch.float32: "f32", torch.float16: "f16", torch.bfloat16: "bf16"}[sess.dtype]
    hist = [PO.History(p, N) for p in prompts]
    logits = sess.prefill(ids, attention_mask=attn)
    out = [[] for _ in range(B)]
    for t in range(T):
        raw = PO.to_native(logits)
        tok = []
        for b in range(B):
            adj = PO.penalize(raw[b], dt, hist[b].P, hist[b].G, *settings[b], bias=biases[b])
            tok.append(PO.argmax_low(adj, dt))
            out[b].append(tok[-1])
            hist[b].count(tok[-1])
        if t + 1 < T:
            logits = sess.decode_step(torch.tensor(tok, dtype=torch.long, device=dev)[:, None], greedy=False)
    return out


def test_generate_ids_greedy_equals_the_loop(tiny_f32):
    model, cfg = tiny_f32
    p = [17, 3, 99, 250, 8, 61]
    T = 24
    dec = ChatGLMDecoder(cfg, model)
    base = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    assert dec.last_stats["penalties"] is False
    banned = base[0]
    kw = dict(repetition_penalty=1.4, frequency_penalty=0.3, logit_bias={banned: NINF, base[1]: -0.5})
    got = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, **kw))
    assert dec.last_stats["penalties"] is True
    want = loop_tokens(model, [p], T, [(1.4, 0.0, 0.3)], [kw["logit_bias"]])[0]
    assert got == want
    assert banned not in got and got != base
    # a presence penalty alone, and the host-sampled path with everything on (repeatable under torch.manual_seed, banned id absent)
    got_p = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, presence_penalty=1.5))
    assert got_p == loop_tokens(model, [p], T, [(1.0, 1.5, 0.0)], [None])[0]
    torch.manual_seed(5)
    a = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, presence_penalty=0.5, **kw))
    torch.manual_seed(5)
    assert a == list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, presence_penalty=0.5, **kw))
    assert banned not in a and len(a) == T


def test_generate_batch_ids_per_row_equals_the_loop_and_pads_are_no_prompt_tokens(tiny_f32):
    model, cfg = tiny_f32
    # row 1 is short and holds no 0 (the pad id) among its real ids; row 0 is the longer prompt next to it
    prompts = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0]]
    T = 16
    dec = ChatGLMDecoder(cfg, model)
    base = dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True)
    banned = base[2][0]
    r, p, f = [1.5, 1.0, 1.2], [0.0, 0.7, 0.0], [0.4, 0.0, 0.1]
    bias = [None, {base[1][0]: -1.0}, {banned: NINF}]
    got = dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True, repetition_penalty=r,
                                 presence_penalty=p, frequency_penalty=f, logit_bias=bias)
    assert dec.last_stats["penalties"] is True
    want = loop_tokens(model, prompts, T, list(zip(r, p, f)), bias)
    assert got == want
    assert banned not in got[2] and got != base
    pen = dec._batch_sessions[3][1].pen
    flagged = [set(torch.nonzero(pen.counts[b, :cfg.vocab_size] < 0).view(-1).tolist()) for b in range(3)]
    assert flagged == [set(p_) for p_ in prompts] and 0 not in flagged[0] and 0 not in flagged[1] and 0 in flagged[2]
    assert pen.generated().sum(dim=1).tolist() == [T - 1] * 3    # the last token of a row is never fed back
    # a scalar serves every row; one row's settings do not move another row
    one = dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True, repetition_penalty=[1.0, 1.0, 1.2],
                                 frequency_penalty=[0.0, 0.0, 0.1], logit_bias=[None, None, {banned: NINF}])
    assert one[0] == base[0] and one[1] == base[1] and one[2] == got[2]
    same = dec.generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True, repetition_penalty=1.5)
    assert same == loop_tokens(model, prompts, T, [(1.5, 0.0, 0.0)] * 3, [None] * 3)


def test_defaults_take_todays_path(tiny_f32):
    model, cfg = tiny_f32
    p = [17, 3, 99, 250]
    prompts = [[5, 9, 200], [44, 3]]
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=10, ignore_eos=True)
    off = dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, logit_bias=None)
    assert list(dec.generate_ids(p, greedy=True, **kw, **off)) == list(dec.generate_ids(p, greedy=True, **kw))
    torch.manual_seed(3)
    a = list(dec.generate_ids(p, **kw))
    torch.manual_seed(3)
    assert list(dec.generate_ids(p, logit_bias={}, **kw)) == a
    assert dec.generate_batch_ids(prompts, seed=[1, 2], **kw, **off) == dec.generate_batch_ids(prompts, seed=[1, 2], **kw)
    assert dec.last_stats["penalties"] is False
    assert dec._session.pen is None and dec._batch_sessions[2][1].pen is None       # never armed: nothing allocated


def test_api_argument_errors(tiny_f32):
    model, cfg = tiny_f32
    dec = ChatGLMDecoder(cfg, model)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan")), dict(presence_penalty=float("nan")),
               dict(frequency_penalty=float("inf")), dict(logit_bias={3: float("inf")}), dict(logit_bias={3: float("nan")}),
               dict(logit_bias={cfg.vocab_size: 1.0}), dict(logit_bias={i: 0.0 for i in range(fused_ops.LOGIT_BIAS_MAX + 1)})):
        with pytest.raises(ValueError):
            list(dec.generate_ids([1, 2, 3], max_generated_tokens=4, greedy=True, **kw))
        with pytest.raises(ValueError):
            dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=4, greedy=True, **kw)
    for kw in (dict(repetition_penalty=[1.1]), dict(presence_penalty=[0.1, 0.2, 0.3]), dict(frequency_penalty=[0.1]),
               dict(logit_bias=[None, None, None])):
        with pytest.raises(ValueError):
            dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=4, greedy=True, **kw)
    with pytest.raises(ValueError, match="row 1"):
        dec.generate_batch_ids([[1, 2], [3]], max_generated_tokens=4, greedy=True, repetition_penalty=[1.0, -2.0])

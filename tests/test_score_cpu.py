"""Scoring on the session path, CPU branch: ``fused_ops.token_logprob`` (dense formula), ``DecodeSession.score``,
``ChatGLMDecoder.score_ids`` / ``perplexity`` against what the REFERENCE model's ``forward(labels=...)`` produced
(tests/golden/score.npz, generator: tests/golden/make_golden_score.py) and against this package's own ``forward(labels=)``.
The GPU twin (the HIP kernel through the C ABI, the real-width cases) is test_score_gpu.py."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import _golden as G
from oracle import qlinear_oracle as O
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = G.load("score.npz")
# log-prob vectors against the reference: the bars test_model_cpu.py holds the tiny logits to (f32: 2e-4 at the decode step
# against the fixture; f16: 2e-3, one fp16 rounding of a dot product per layer output on another host's BLAS)
TOL = {"f32": 2e-4, "f16": 2e-3}


def case(name):
    return {k: torch.from_numpy(Z[f"{name}/{k}"]) for k in ("ids", "attention_mask", "labels", "logprobs")}, float(Z[f"{name}/loss"])


def logprob64(x, t, ignore_index=-100):
    """float64 restatement: log_softmax gathered at the targets, 0 at ignored ones, NaN outside [0, N)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = x.max(axis=1, keepdims=True)
        m0 = np.where(np.isfinite(m), m, 0.0)
        lse = m0[:, 0] + np.log(np.exp(x - m0).sum(axis=1))
    out = np.empty(len(t))
    for r, tr in enumerate(t):
        out[r] = 0.0 if tr == ignore_index else (x[r, tr] - lse[r] if 0 <= tr < x.shape[1] else np.nan)
    return out, lse


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_token_logprob_cpu_route_against_float64(dtype):
    g = torch.Generator().manual_seed(11)
    x = (torch.randn(9, 777, generator=g) * 4).to(dtype)
    x[3, 5:700] = float("-inf")
    x[4] = float("-inf")
    x[4, 123] = 1.5                                             # one finite entry: probability 1
    t = torch.tensor([0, 776, -100, 5, 123, 777, -1, 10**12, 400])
    lp, lse, am = fused_ops.token_logprob(x, t, return_lse=True, return_argmax=True)
    assert lp.dtype == torch.float32 and lse.dtype == torch.float32 and am.dtype == torch.int64
    want, lse64 = logprob64(x.float().numpy(), t.tolist())
    got = lp.double().numpy()
    assert got[2] == 0.0 and np.isnan(got[[5, 6, 7]]).all()     # ignored -> 0, out of range -> NaN
    assert got[3] == -np.inf and want[3] == -np.inf             # a -inf logit has log-probability -inf, not NaN
    assert got[4] == 0.0
    fin = np.isfinite(want)
    assert np.array_equal(fin, np.isfinite(got))
    assert np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))) < 2e-6
    assert np.max(np.abs(lse.double().numpy() - lse64) / np.maximum(1.0, np.abs(lse64))) < 2e-6
    assert np.array_equal(am.numpy(), x.float().numpy().argmax(axis=1))
    assert torch.allclose(fused_ops.token_logprob(x, t), lp, rtol=0, atol=0, equal_nan=True)   # the single-output form
    # another ignore_index
    assert fused_ops.token_logprob(x, t, ignore_index=776)[1] == 0.0


def test_token_logprob_argument_checks():
    x = torch.zeros(3, 8)
    with pytest.raises(ValueError):
        fused_ops.token_logprob(x[0], torch.zeros(3, dtype=torch.long))
    with pytest.raises(ValueError):
        fused_ops.token_logprob(x, torch.zeros(2, dtype=torch.long))
    with pytest.raises(ValueError):
        fused_ops.token_logprob(x, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError):
        fused_ops.token_logprob(torch.zeros(3, 0), torch.zeros(3, dtype=torch.long))
    assert fused_ops.token_logprob(torch.zeros(0, 8), torch.zeros(0, dtype=torch.long)).shape == (0,)


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_session_score_matches_reference_and_own_forward(dt):
    """The CPU route serves fp16 as well as fp32 (the modules' CPU branch is dtype-generic): both tiny cases run."""
    model, cfg = build(dt)
    c, loss_ref = case(f"tiny/{dt}")
    B, S = c["ids"].shape
    sess = DecodeSession(model, B, 32)
    res = sess.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], return_argmax=True)
    assert res.logprobs.shape == (B, S - 1) and res.logprobs.dtype == torch.float32 and res.loss.dim() == 0
    assert torch.equal(res.valid, c["labels"][:, 1:] != -100) and bool(res.valid.any(dim=1).all())
    assert bool((res.logprobs[~res.valid] == 0).all())
    for b in range(B):
        e = O.rel_l2(res.logprobs[b].numpy(), c["logprobs"][b].numpy())
        print(f"[score cpu] tiny/{dt} row {b}: log-prob rel-L2 vs reference {e:.3e}")
        assert e < TOL[dt]
    print(f"[score cpu] tiny/{dt}: loss {float(res.loss):.6f} reference {loss_ref:.6f}")
    assert abs(float(res.loss) - loss_ref) <= TOL[dt] * abs(loss_ref)
    # this package's own forward(labels=): two routes of one function
    with torch.no_grad():
        loss_fwd, logits, _ = model(input_ids=c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    if dt == "f32":
        assert torch.allclose(res.loss, loss_fwd, atol=1e-5, rtol=1e-5)
        assert torch.equal(res.argmax[res.valid], logits[:, :-1].argmax(-1)[res.valid])
    else:
        assert abs(float(res.loss) - float(loss_fwd)) <= TOL[dt] * abs(float(loss_fwd))
    # default labels = ids with -100 at the pads: the reference tokenizer's return_labels
    sess2 = DecodeSession(model, B, 32)
    res2 = sess2.score(c["ids"], attention_mask=c["attention_mask"])
    want_valid = c["attention_mask"][:, 1:].bool()
    assert torch.equal(res2.valid, want_valid)
    both = res.valid & want_valid
    assert torch.equal(res2.logprobs[both], res.logprobs[both])


@pytest.mark.parametrize("dt", ["f32", "f16"])
def test_chunked_score_equals_unchunked(dt):
    """chunk = 5 and head_rows = 3 split the 14 positions and the 3 x 5 rows of a chunk unevenly.  Compared: every entry whose
    QUERY position holds a token.  The one entry per padded row whose query is the last pad (it scores the row's first token,
    as the reference's labels ask) is no function of the sequence: a pad's attention row is masked everywhere, i.e. uniform
    over every key of the forward pass it runs in - the whole padded width in one pass (what the fixture records and the
    unchunked call reproduces), the keys so far in a chunked one; the reference's own forward with past_key_values differs
    from its one-pass forward in the same entries.  Those entries must be finite, nothing more can be asked of them."""
    model, cfg = build(dt)
    c, _ = case(f"tiny/{dt}")
    B = c["ids"].shape[0]
    whole = DecodeSession(model, B, 32).score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    parts = DecodeSession(model, B, 32).score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], chunk=5, head_rows=3)
    assert torch.equal(parts.valid, whole.valid)
    real_query = c["attention_mask"][:, :-1].bool()
    assert int((whole.valid & ~real_query).sum()) == 1            # row 2's; row 1 is padded too, but its first tokens are a -100 span
    assert bool(torch.isfinite(parts.logprobs).all())
    for b in range(B):
        e = O.rel_l2(parts.logprobs[b][real_query[b]].numpy(), whole.logprobs[b][real_query[b]].numpy())
        print(f"[score cpu] tiny/{dt} row {b}: chunked vs unchunked rel-L2 {e:.3e}")
        assert e < TOL[dt]
    sel = whole.valid & real_query
    la, lb = -parts.logprobs[sel].double().mean(), -whole.logprobs[sel].double().mean()
    assert abs(float(la) - float(lb)) <= TOL[dt] * abs(float(lb))


def test_score_then_decode_equals_prefill_then_decode_bitwise():
    model, cfg = build("f32")
    c, _ = case("tiny/f32")
    B = c["ids"].shape[0]
    a, b = DecodeSession(model, B, 32), DecodeSession(model, B, 32)
    last_a = a.prefill(c["ids"], attention_mask=c["attention_mask"])
    res = b.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], chunk=5, head_rows=4)
    last_a5 = DecodeSession(model, B, 32).prefill(c["ids"], chunk=5, attention_mask=c["attention_mask"])
    assert torch.equal(res.logits, last_a5)                      # the same chunking: the same bits
    b2 = DecodeSession(model, B, 32)
    res2 = b2.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    assert torch.equal(res2.logits, last_a)
    for name in ("write_index", "pos", "mask", "pad_cols", "n_tokens"):
        assert torch.equal(getattr(a, name), getattr(b2, name)), name
    assert a.length == b2.length and a.cache.length == b2.cache.length
    a.tok.copy_(last_a.argmax(-1, keepdim=True))
    b2.tok.copy_(res2.logits.argmax(-1, keepdim=True))
    for _ in range(2):
        la, lb = a.decode_step(greedy=True), b2.decode_step(greedy=True)
        assert torch.equal(la, lb) and torch.equal(a.tok, b2.tok)


def test_step_return_hidden_feeds_head():
    model, cfg = build("f32")
    ids = torch.from_numpy(Z["tiny/f32/ids"])[:1, -6:]
    cap, S = 16, ids.shape[1]
    t = torch.arange(cap)
    mask = ((t[None, :] > torch.arange(S)[:, None]).float() * -1e10)[None]
    pos = torch.arange(1, S + 1)[None]
    with torch.no_grad():
        logits = model.step(ids, model.new_cache(1, cap), torch.arange(S), pos, mask)
        hidden = model.step(ids, model.new_cache(1, cap), torch.arange(S), pos, mask, return_hidden=True)
        last = model.step(ids, model.new_cache(1, cap), torch.arange(S), pos, mask, last_only=True, return_hidden=True)
    assert hidden.shape == (1, S, cfg.hidden_size) and last.shape == (1, 1, cfg.hidden_size)
    assert torch.equal(model.head(hidden), logits) and torch.equal(last, hidden[:, -1:])


def test_score_ids_and_perplexity_plumbing():
    model, cfg = build("f32")
    dec = ChatGLMDecoder(cfg, model)
    g = torch.Generator().manual_seed(5)
    seqs = [torch.randint(1, cfg.vocab_size, (n,), generator=g).tolist() for n in (9, 4, 1, 12)]
    lps, loss = dec.score_ids(seqs)
    assert [len(l) for l in lps] == [8, 3, 0, 11]
    # every sequence alone through forward(labels=): left padding does not change a sequence's numbers
    total, count = 0.0, 0
    for s, lp in zip(seqs, lps):
        if len(s) < 2:
            continue
        ids = torch.tensor([s])
        with torch.no_grad():
            _, logits, _ = model(input_ids=ids)
        want = torch.log_softmax(logits[0, :-1].float(), -1).gather(1, ids[0, 1:, None])[:, 0]
        assert torch.allclose(torch.tensor(lp), want, atol=1e-5, rtol=1e-5)
        total, count = total + float(want.sum()), count + len(lp)
    assert abs(loss - (-total / count)) < 1e-5
    sess = dec._batch_sessions[4][1]
    lps2, loss2 = dec.score_ids(seqs)
    assert dec._batch_sessions[4][1] is sess and lps2 == lps and loss2 == loss     # reused, not rebuilt
    # labels: a prompt span is not scored
    labels = [list(s) for s in seqs]
    labels[0][:5] = [-100] * 5
    lps3, loss3 = dec.score_ids(seqs, labels=labels)
    assert lps3[0][:4] == [0.0] * 4 and lps3[0][4:] == lps[0][4:] and lps3[1] == lps[1]
    # reference_labels: the loss the reference's forward(labels=) gives the left-padded batch (first tokens scored from a pad)
    S = max(len(s) for s in seqs)
    ids, attn = torch.zeros(4, S, dtype=torch.long), torch.zeros(4, S, dtype=torch.long)
    for b, s in enumerate(seqs):
        ids[b, S - len(s):], attn[b, S - len(s):] = torch.tensor(s), 1
    with torch.no_grad():
        loss_fwd, _, _ = model(input_ids=ids, attention_mask=attn, labels=ids.masked_fill(~attn.bool(), -100))
    lps4, loss4 = dec.score_ids(seqs, reference_labels=True)
    assert lps4 == lps and abs(loss4 - float(loss_fwd)) < 1e-5
    # perplexity: exp of the MEAN OF THE BATCH LOSSES (examples/evaluations/ppl.py), not of the token mean
    batches = [seqs[:2], seqs[3:]]
    losses = [dec.score_ids(bt)[1] for bt in batches]
    assert abs(dec.perplexity(batches) - math.exp(sum(losses) / 2)) < 1e-9
    # generation still gets its own batch-1 session
    list(dec.generate_ids(seqs[0][:4], max_generated_tokens=2, greedy=True))
    assert dec._session.batch == 1 and dec._batch_sessions[4][1] is sess
    with pytest.raises(ValueError):
        dec.score_ids([[1, 2], []])
    with pytest.raises(RuntimeError):
        dec.score("text")

    class Tok:
        def encode(self, text):
            return [1 + ord(ch) % 200 for ch in text]
    dec.tokenizer = Tok()
    one, _ = dec.score("hello world")
    assert len(one) == 10
    many, _ = dec.score(["hello", "hi there"])
    assert [len(m) for m in many] == [4, 7]


def test_header_declares_and_library_exports_token_logprob():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"\bint\s+qlinear_token_logprob\s*\(", header)
    assert re.search(r"#define\s+QLINEAR_ABI_VERSION\s+3\b", header)
    assert "qlinear_token_logprob" in _lib.EXPORTS
    assert _lib.available(), "libqlinear_hip.so must be built (python -c 'import __graft_entry__ as g; g.build()')"
    assert getattr(ctypes.CDLL(_lib.LIB_PATH), "qlinear_token_logprob") is not None
    assert getattr(ctypes.CDLL(_lib.DEV_LIB_PATH), "qlinear_token_logprob") is not None
    # the checks that need no device: status codes, and R == 0 is QL_OK without a launch
    lib = _lib.get_lib()
    before = _lib.launch_count()
    assert lib.qlinear_token_logprob(None, 0, 8, 8, None, -100, None, None, None, 1, None) == 0
    assert _lib.launch_count() == before
    assert lib.qlinear_token_logprob(None, 2, 8, 8, None, -100, None, None, None, 1, None) == -1      # QL_ERR_NULL_POINTER
    assert lib.qlinear_token_logprob(None, 2, 8, 7, None, -100, None, None, None, 1, None) == -2      # ldl < N
    assert lib.qlinear_token_logprob(None, 2, 0, 8, None, -100, None, None, None, 1, None) == -2
    assert lib.qlinear_token_logprob(None, 2, 8, 8, None, -100, None, None, None, 9, None) == -3      # dtype

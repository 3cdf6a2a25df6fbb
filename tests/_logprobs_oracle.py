"""What tests/test_gen_logprobs_cpu.py and tests/test_gen_logprobs_gpu.py compare ``fused_ops.step_logprobs`` and the decoders'
``logprobs=`` with: a numpy float64 log_softmax, the strict total order (value descending, index ascending, NaN as -inf) as a stable
arg-sort of the negated row, and a teacher-forced eager loop over a model that hands back the logits every token was selected from."""
import numpy as np
import torch

from chatglm_q_amd import fused_ops
from chatglm_q_amd.decoder import DecodeSession


def log_softmax64(x):
    """Rows of log_softmax in float64, relative to the row maximum (x: array (..., N) of any float dtype)."""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.max(np.where(np.isnan(x), -np.inf, x), axis=-1, keepdims=True)
        m = np.where(np.isfinite(m), m, 0.0)
        return (x - m) - np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True))


def order(row):
    """Indices of one row under (value descending, index ascending); a NaN ranks as -inf."""
    v = np.asarray(row, dtype=np.float64)
    v = np.where(np.isnan(v), -np.inf, v)
    return np.argsort(-v, kind="stable")


def top(row, n):
    """(ids, float64 log-probs) of the n first entries of ``order(row)``, padded with (-1, -inf) past the row's length."""
    N = len(row)
    idx = order(row)[:min(n, N)]
    lp = log_softmax64(row)[idx]
    pad = n - len(idx)
    return (np.concatenate([idx, np.full(pad, -1, dtype=idx.dtype)]).astype(np.int64),
            np.concatenate([lp, np.full(pad, -np.inf)]))


def metric(got, want):
    """tests/test_score_gpu.py's: max |got - want| / max(1, |want|) over the finite entries of `want`; the others agree exactly."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN pattern"
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "infinities"
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


def replay_logits(model, prompts, tokens, settings=None, biases=None, pad_id=0):
    """The test's own loop in the eager "logits" mode, teacher-forced with ``tokens`` (one list per prompt, any lengths): prefill
    the left-padded batch, adjust every step's logits with ``fused_ops.logit_penalties`` (``settings`` / ``biases`` per row, or
    None), feed row b's token t (its last one once it has run out).  Returns one (B, vocab) tensor per step: the logits token t
    of every row was selected from."""
    B, S, N = len(prompts), max(len(p) for p in prompts), model.config.vocab_size
    T = max(len(t) for t in tokens)
    ids = torch.full((B, S), pad_id, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    dev = model.final_ln.weight.device
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    pen = None
    if settings is not None:
        pen = fused_ops.PenaltyState(B, N, dev).arm(prompts, settings, biases)
    logits = sess.prefill(ids, attention_mask=attn)
    rows, fed = [], None
    for t in range(T):
        lg = logits.contiguous().clone()
        if pen is not None:
            fused_ops.logit_penalties(lg, pen, fed)
        rows.append(lg)
        fed = torch.tensor([tk[min(t, len(tk) - 1)] if tk else 0 for tk in tokens], dtype=torch.long, device=dev)
        if t + 1 < T:
            logits = sess.decode_step(fed[:, None], greedy=False)
    return rows


def check_record(rows, tokens, records, n, exact=True):
    """Every row's record against the replayed logits: as long as its tokens; token t's log-prob and the n alternatives' equal
    ``fused_ops.token_logprob`` on step t's logits at those ids (bit for bit), the alternatives' ids equal ``order``'s."""
    B = len(tokens)
    dev = rows[0].device
    for b in range(B):
        rec = records[b]
        assert len(rec.token_logprobs) == len(rec.top_ids) == len(rec.top_logprobs) == len(tokens[b]), (b, len(rec.token_logprobs), len(tokens[b]))
    for t, lg in enumerate(rows):
        live = [b for b in range(B) if t < len(tokens[b])]
        if not live:
            continue
        tgt = torch.tensor([tokens[b][t] if t < len(tokens[b]) else 0 for b in range(B)], dtype=torch.long, device=dev)
        want = fused_ops.token_logprob(lg, tgt).cpu()
        host = lg.float().cpu().numpy()
        for b in live:
            got = torch.tensor(records[b].token_logprobs[t], dtype=torch.float32)
            assert torch.allclose(got, want[b], rtol=0, atol=0, equal_nan=True), (b, t, float(got), float(want[b]))
            assert records[b].top_ids[t] == order(host[b])[:n].tolist(), (b, t)
        for j in range(n):
            tj = torch.tensor([records[b].top_ids[t][j] if t < len(tokens[b]) else 0 for b in range(B)], dtype=torch.long, device=dev)
            wj = fused_ops.token_logprob(lg, tj).cpu()
            for b in live:
                got = torch.tensor(records[b].top_logprobs[t][j], dtype=torch.float32)
                assert torch.allclose(got, wj[b], rtol=0, atol=0, equal_nan=True), (b, t, j, float(got), float(wj[b]))

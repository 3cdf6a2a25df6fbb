"""Scenarios shared by the CPU and GPU beam search tests: random candidate lists on a coarse grid of log-probs (sums are exact in fp32,
so exact score ties across rows are common), driven through ``fused_ops.beam_advance`` and the Python oracle side by side with every
buffer compared as bit patterns after every step; and the ``beam_gather`` cases against ``index_select`` on clones."""
import random

import numpy as np
import torch

import _beam_oracle as BO
from chatglm_q_amd import fused_ops


# (P, B, length_penalty, early_stopping) of the advance scenarios; test_beam_cpu asserts that together they meet every case of the rules
CONFIGS = [(3, 2, 0.0, False), (3, 4, 0.0, False), (3, 2, 1.0, True), (1, 10, 2.5, False), (1, 1, 1.0, True), (3, 4, 2.5, False),
           (1, 4, 1.0, False), (3, 10, 1.0, True), (3, 1, 0.0, False), (1, 2, 2.5, True)]


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).numpy() if t.dtype == torch.float32 else t.numpy()


def fbits(values):
    return np.array(values, dtype=np.float32).view(np.int32)


def random_candidates(rng, R, B, eos, vocab=50, p_end=0.7):
    """(ids, lps) (R, 2B): distinct ids per row, log-probs descending on a grid of 0.25; the end id at a random rank in some rows."""
    W = 2 * B
    ids, lps = [], []
    for _ in range(R):
        row = rng.sample([i for i in range(vocab) if i != eos], W)
        if eos is not None and eos >= 0 and rng.random() < p_end:
            row[min(rng.randrange(W), rng.randrange(W), rng.randrange(W))] = eos          # mostly near the front
        lp = sorted((-0.25 * rng.randrange(1, 12) for _ in range(W)), reverse=True)
        ids.append(row)
        lps.append(lp)
    return ids, lps


def state_matches(st, oracle, tok):
    """Every buffer of the BeamState against the oracle, floats as bit patterns."""
    P, B, R = oracle.P, oracle.B, oracle.P * oracle.B
    h = st.fetch()
    assert tok.cpu().view(-1).tolist() == oracle.tok
    assert h["parent"].tolist() == oracle.parent
    assert np.array_equal(bits(h["beam_score"]), fbits(oracle.score))
    assert h["steps"][:P].tolist() == oracle.steps
    assert h["done"][:P].tolist() == [int(d) for d in oracle.done]
    assert h["live"].tolist() == [oracle.live]
    assert h["fin_count"][:P].tolist() == [len(q) for q in oracle.heap]
    for g in range(P):
        n = len(oracle.heap[g])
        sl = slice(g * B, g * B + n)
        assert np.array_equal(bits(h["fin_score"][sl]), fbits([e[0] for e in oracle.heap[g]]))
        assert np.array_equal(bits(h["fin_sum"][sl]), fbits([e[3] for e in oracle.heap[g]]))
        assert h["fin_len"][sl].tolist() == [e[1] for e in oracle.heap[g]]
        assert h["fin_row"][sl].tolist() == [e[2] for e in oracle.heap[g]]
        for s in range(oracle.steps[g]):
            for r in range(g * B, g * B + B):
                assert tuple(h["trellis"][s, r].tolist()) == oracle.trellis[(s, r)], (s, r)
    assert st.cand.count.cpu().tolist() == [0] * R
    assert np.array_equal(bits(st.norm), oracle.norm.view(np.int32))


def run_scenario(device, P, B, eos, length_penalty, early, n_steps, cap, seed, book=False, capacity=16):
    """Drive ``n_steps`` advances through fused_ops and the oracle; returns the oracle (its ``events`` say what the rules met)."""
    rng = random.Random(seed)
    R = P * B
    st = fused_ops.BeamState(R, cap, device).arm(P, B, eos, length_penalty, early, first=3)
    oracle = BO.Beams(P, B, eos, length_penalty, early, cap)
    tok = torch.full((R,), 7, dtype=torch.int64, device=device)
    if book:
        wi = torch.tensor([5], dtype=torch.int64, device=device)
        pos = torch.arange(R, dtype=torch.int64, device=device) + 2
        mask = torch.full((R, 1, capacity), -1e10, dtype=torch.float32, device=device)
    for step in range(n_steps):
        ids, lps = random_candidates(rng, R, B, eos)
        st.cand.top_ids.copy_(torch.tensor(ids, dtype=torch.int32).view(R, 1, 2 * B))
        st.cand.top_lp.copy_(torch.tensor(lps, dtype=torch.float32).view(R, 1, 2 * B))
        st.cand.count.fill_(1)
        if book:
            before = mask.clone()
            fused_ops.beam_advance(st, tok, wi, pos, mask)
            nw = 5 + step + 1
            assert wi.tolist() == [nw] and pos.tolist() == [r + 2 + step + 1 for r in range(R)]
            if nw < capacity:
                before[:, :, nw] = 0.0
            assert torch.equal(mask, before)
        else:
            fused_ops.beam_advance(st, tok)
        oracle.advance(ids, lps)
        state_matches(st, oracle, tok)
    return oracle


# ---- gather ---------------------------------------------------------------------------------------------------------------------------
MARGIN = 64                                                      # sentinel elements in front of and behind every buffer


def gather_parents(kind, P, B, rng):
    """(parent rows, rows index_select reads): ``kind`` identity / first (broadcast) / cycle (a 3-cycle, B >= 3; a swap at B = 2) /
    dup (duplicates) / outside (a value outside the row's group, which must clamp)."""
    parent, src = [], []
    for g in range(P):
        r0 = g * B
        if kind == "identity":
            loc = list(range(B))
        elif kind == "first":
            loc = [0] * B
        elif kind == "cycle":
            loc = list(range(B))
            if B >= 3:
                loc[0], loc[1], loc[2] = 1, 2, 0
            else:
                loc[0], loc[1] = 1, 0
        elif kind == "dup":
            loc = [rng.randrange(B) for _ in range(B)]
            loc[B - 1] = loc[0]
        else:
            loc = [rng.randrange(B) for _ in range(B)]
        p = [r0 + v for v in loc]
        s = list(p)
        if kind == "outside":
            p[0], s[0] = r0 + B + 3, r0 + B - 1                  # above the group: clamps to its last row
            p[B - 1], s[B - 1] = r0 - 2, r0                      # below the group: clamps to its first row
        parent += p
        src += s
    return parent, src


def run_gather(device, P, B, capacity, tail, dtype, kind, first, end, n_buf=3, seed=0):
    """``n_buf`` buffers (R, capacity, *tail) carved out of sentinel-padded storage; gather; compare with index_select on clones -
    everything outside [first, end) and the margins bit-unchanged."""
    rng = random.Random(seed)
    g = torch.Generator().manual_seed(seed)
    R = P * B
    n = R * capacity * int(np.prod(tail))
    raw = [torch.randint(-30000, 30000, (n + 2 * MARGIN,), generator=g, dtype=torch.int32).to(torch.int16).view(torch.float16)
           if dtype == torch.float16 else torch.randn(n + 2 * MARGIN, generator=g) for _ in range(n_buf)]
    raw = [t.to(device) for t in raw]
    bufs = [t[MARGIN:MARGIN + n].view(R, capacity, *tail) for t in raw]
    want = [t.clone() for t in raw]
    parent, src = gather_parents(kind, P, B, rng)
    lo, hi = max(first, 0), min(end, capacity)
    if lo < hi:
        for w in want:
            v = w[MARGIN:MARGIN + n].view(R, capacity, *tail)
            v[:, lo:hi] = v.index_select(0, torch.tensor(src, device=device))[:, lo:hi].clone()
    table = fused_ops.BeamGatherTable(bufs)
    fused_ops.beam_gather(table, torch.tensor(parent, dtype=torch.int32, device=device), torch.tensor([first], dtype=torch.int32, device=device),
                          torch.tensor([end], dtype=torch.int64, device=device), B)
    for got, w in zip(raw, want):
        a, b = got.cpu(), w.cpu()
        assert torch.equal(a.view(torch.int16) if dtype == torch.float16 else a.view(torch.int32),
                           b.view(torch.int16) if dtype == torch.float16 else b.view(torch.int32))

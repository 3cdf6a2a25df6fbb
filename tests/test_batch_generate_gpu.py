"""Batched generation on the GPU: ``qlinear_batch_sample_advance`` (csrc/sampler.hip) through ``fused_ops`` / ctypes against the
oracle's restatement of the reference sampler, ``qlinear_top_p_sample`` and ``qlinear_greedy_advance``; the captured "rows" step of
``DecodeSession`` and ``ChatGLMDecoder.generate_batch_ids`` against the REFERENCE model's greedy continuation of left-padded
batches (tests/golden/batch_generate.npz), against teacher-forced logits of the same batch, against ``generate_ids`` and against
themselves (graph / eager, row permutations, mode switches, low footprint)."""
import ctypes

import numpy as np
import pytest
import torch

import _golden as G
import _philox
import _sampler_cases as SC
from oracle import qlinear_oracle as O
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny
from test_model_gpu import TINY_TOL
from test_model_real_cpu import build_real
from test_model_real_gpu import TOL as REAL_TOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Z = G.load("batch_generate.npz")
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def rows_of(B, out_ld, params, seeds, budgets, stop=None, ctrs=None):
    r = fused_ops.BatchRows(B, out_ld, DEV).arm(params, seeds, budgets, stop)
    if ctrs is not None:
        r.row_rng[:, 1] = torch.tensor(ctrs, dtype=torch.int64, device=DEV)
    return r


def inverse_cdf_ok(tok, probs, idx, u):
    """The token is the inverse CDF of the row's filtered distribution at u (u within rounding of a CDF step: either neighbour),
    the allowance of test_sampler_gpu.py."""
    k = len(probs)
    cdf = np.cumsum(probs.astype(np.float64))
    j = int(np.searchsorted(cdf, float(u) * cdf[-1], side="right"))
    j = min(j, int((probs > 0).sum()) - 1)
    near = [idx[jj] for jj in (j - 1, j, j + 1) if 0 <= jj < k]
    edge = min(abs(float(u) * cdf[-1] - c) for c in cdf[max(0, j - 1): j + 1])
    return tok == idx[j] or (edge < 1e-6 and tok in near)


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1000, 65024, 65025])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_distribution_per_row_vs_oracle(N, dt):
    """Per-row parameters mixed inside one launch: each row's filtered distribution equals the oracle's index for index (1e-6), u is
    the Philox number of (seed_b, ctr_b, 0) and the token the inverse CDF at u."""
    combos = [(k, p, t) for k in (1, 7, 100, 1024) for p in (0.3, 0.8, 1.0) for t in (0.5, 1.0, 1.7)]
    B = len(combos)
    g = torch.Generator().manual_seed(N + len(dt))
    lg = (torch.randn(B, N, generator=g) * 3).to(TDT[dt]).to(DEV)
    seeds = [1000 + 17 * b for b in range(B)]
    ctrs = [3 * b for b in range(B)]
    rows = rows_of(B, 4, combos, seeds, [4] * B, ctrs=ctrs)
    tok = torch.full((B,), -1, dtype=torch.int64, device=DEV)
    probs, idx, u = fused_ops.batch_sample_advance(lg, tok, rows, return_distribution=True)
    torch.cuda.synchronize()
    x = lg.float().cpu().numpy()
    probs, idx, u, tok = probs.cpu().numpy(), idx.cpu().numpy(), u.cpu().numpy(), tok.cpu().numpy()
    rng = rows.row_rng.cpu().numpy()
    for b, (k, p, t) in enumerate(combos):
        want_p, want_i = O.top_p_filter(x[b], k, p, t)
        kk = min(k, N)
        assert np.array_equal(idx[b, :kk], want_i), (dt, N, combos[b])
        np.testing.assert_allclose(probs[b, :kk], want_p, rtol=0, atol=1e-6)
        assert u[b] == _philox.uniform(seeds[b], ctrs[b], 0)
        assert inverse_cdf_ok(tok[b], probs[b, :kk], idx[b, :kk], u[b]), (dt, N, combos[b], tok[b])
        assert rng[b, 0] == seeds[b] and rng[b, 1] == ctrs[b] + 1
    assert rows.out_tokens[:, 0].cpu().numpy().tolist() == tok.tolist()
    assert rows.row_state.cpu().numpy().tolist() == [[1, 0]] * B and int(rows.live[0]) == B


def test_greedy_rows_equal_greedy_advance_bit_for_bit():
    g = torch.Generator().manual_seed(78)
    for dtype in (torch.float16, torch.bfloat16, torch.float32):
        lg = (torch.randn((5, 65024), generator=g) * 3).to(dtype).to(DEV)
        lg[1, 100] = lg[1].max() + 1; lg[1, 60000] = lg[1, 100]               # a tie for the maximum: lowest index wins in both
        lg[3, 64999] = lg[3].max() + 1; lg[3, 65020] = lg[3, 64999]           # ... in the last chunks as well
        cap = 64

        def state():
            return (torch.zeros(5, 1, dtype=torch.int64, device=DEV), torch.full((1,), 7, dtype=torch.int64, device=DEV),
                    torch.arange(5, dtype=torch.int64, device=DEV)[:, None].contiguous(),
                    torch.full((5, 1, cap), -1e10, dtype=torch.float32, device=DEV))
        tg, wg, pg, mg = state()
        fused_ops.greedy_advance(lg, tg, wg, pg, mg)
        ts, ws, ps, ms = state()
        rows = rows_of(5, 8, [(1, 0.8, 1.0)] * 5, [1, 2, 3, 4, 5], [8] * 5)
        fused_ops.batch_sample_advance(lg, ts.view(-1), rows, ws, ps.view(-1), ms)
        torch.cuda.synchronize()
        for a, b in ((tg, ts), (wg, ws), (pg, ps), (mg, ms)):
            assert torch.equal(a, b)
        assert ts[1, 0] == 100 and ts[3, 0] == 64999
        assert torch.equal(rows.out_tokens[:, 0], ts.view(-1))


@pytest.mark.parametrize("temperature", [1.0, 0.7])
def test_single_row_equals_top_p_sample(temperature):
    """One row over 64 counters: token, u and distribution equal qlinear_top_p_sample's exactly."""
    name = "vocab_default"
    _, N, _, dtype, top_k, top_p, _ = SC.CASES[name]
    lg = torch.from_numpy(SC.logits_for(name)).to(TDT[dtype]).to(DEV)[None].contiguous()
    t1 = torch.zeros(1, dtype=torch.int64, device=DEV)
    rng = fused_ops.new_rng_state(1, 4242, DEV)
    t2 = torch.zeros(1, dtype=torch.int64, device=DEV)
    rows = rows_of(1, 64, [(top_k, top_p, temperature)], [4242], [64])
    for c in range(64):
        p1, i1, u1 = fused_ops.top_p_sample(lg, t1, rng, top_k, top_p, temperature, return_distribution=True)
        p2, i2, u2 = fused_ops.batch_sample_advance(lg, t2, rows, return_distribution=True)
        torch.cuda.synchronize()
        k = p1.shape[1]
        assert int(t1) == int(t2) and torch.equal(u1, u2), c
        assert torch.equal(p1, p2[:, :k]) and torch.equal(i1, i2[:, :k]) and not bool(p2[:, k:].any()), c
    assert int(rows.row_rng[0, 1]) == 64 and int(rng[1]) == 64
    assert int(rows.live[0]) == 0 and rows.row_state[0].tolist() == [64, 1]


def test_stop_budget_fill_invalid_and_live():
    B, N = 6, 1000
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, N, generator=g) * 2
    x[0, 5] = 100.0                                             # greedy row 0 hits the stop id at once
    x[2, 10] = float("nan")                                     # a NaN in a sampled row
    x[3] = float("-inf")                                        # an all -inf row
    x[1, 5] = -100.0
    x[4, 5] = -100.0
    lg = x.half().to(DEV)
    params = [(1, 0.8, 1.0), (50, 0.8, 1.0), (100, 0.8, 1.0), (100, 0.8, 1.0), (50, 0.9, 1.3), (1, 0.8, 1.0)]
    rows = rows_of(B, 16, params, list(range(10, 10 + B)), [9, 2, 9, 9, 9, 9], stop=5)
    rows.row_params[5, 2] = 0.0                                 # the kernel's own guard: a non-positive temperature is an invalid row
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    cap = 32
    widx = torch.zeros(1, dtype=torch.int64, device=DEV)
    pos = torch.arange(B, dtype=torch.int64, device=DEV)
    mask = torch.full((B, 1, cap), -1e10, dtype=torch.float32, device=DEV)
    lives = []
    snap = None
    for launch in range(3):
        fused_ops.batch_sample_advance(lg, tok, rows, widx, pos, mask)
        torch.cuda.synchronize()
        lives.append(int(rows.live[0]))
        if launch == 0:
            snap = (rows.row_state.clone(), rows.row_rng.clone(), rows.out_tokens.clone())
            first = tok.cpu().tolist()
    xf = lg.float().cpu()
    assert first[0] == 5
    want2 = int(torch.where(torch.isnan(xf[2]), torch.full_like(xf[2], float("-inf")), xf[2]).argmax())
    assert first[2] == want2 and first[3] == 0 and first[5] == int(xf[5].argmax())
    assert all(0 <= t < N for t in first)
    st = rows.row_state.cpu()
    assert st[0].tolist() == [1, 1] and st[2].tolist() == [1, 3] and st[3].tolist() == [1, 3] and st[5].tolist() == [1, 3]
    assert st[1].tolist() == [2, 1] and st[4].tolist() == [3, 0]                # budget 2 ended row 1, row 4 is live
    assert lives == [2, 1, 1]
    for b in (0, 2, 3, 5):                                      # finished rows: counter, tokens and state untouched
        assert torch.equal(rows.row_state[b], snap[0][b]) and torch.equal(rows.row_rng[b], snap[1][b])
        assert torch.equal(rows.out_tokens[b], snap[2][b])
    assert int(rows.row_rng[4, 1]) == 3 and int(rows.row_rng[1, 1]) == 2
    final = tok.cpu().tolist()
    assert final[0] == final[1] == final[2] == final[3] == final[5] == 5          # the fill id: the stop id
    assert int(widx[0]) == 3 and pos.cpu().tolist() == [b + 3 for b in range(B)]
    assert bool((mask[:, 0, 1:4] == 0).all()) and bool((mask[:, 0, 4:] == -1e10).all())
    # no stop id: a finished row's fill token is its last token
    rows2 = rows_of(2, 4, [(1, 0.8, 1.0)] * 2, [1, 2], [1, 3])
    t2 = torch.zeros(2, dtype=torch.int64, device=DEV)
    fused_ops.batch_sample_advance(lg[:2], t2, rows2)
    last0 = int(t2[0])
    lg2 = lg[:2].flip(1).contiguous()                           # other logits: a live row would pick another token
    fused_ops.batch_sample_advance(lg2, t2, rows2)
    torch.cuda.synchronize()
    assert int(t2[0]) == last0 and int(rows2.out_tokens[0, 0]) == last0 and rows2.row_state[0].tolist() == [1, 1]
    assert rows2.row_state[1].tolist() == [2, 0] and int(rows2.live[0]) == 1


def test_argument_errors_return_status_codes():
    lib = _lib.get_lib()
    B, N = 2, 100
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    rows = rows_of(B, 4, [(1, 0.8, 1.0)] * B, [1, 2], [4, 4])
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    f16 = _lib.dtype_code(torch.float16)

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, out_ld=4, stop=-1, dtype=f16, row_params=rows.row_params.data_ptr(),
             probs=0, idx=0, dist_ld=0, widx=0, pos=0, mask=0):
        return lib.qlinear_batch_sample_advance(logits, b, n, ldl, row_params, rows.row_rng.data_ptr(), rows.row_state.data_ptr(),
                                                rows.budget.data_ptr(), rows.out_tokens.data_ptr(), out_ld, rows.live.data_ptr(), stop,
                                                tok.data_ptr(), widx, pos, mask, 0, probs, idx, 0, dist_ld, dtype,
                                                _lib.stream_ptr(lg.device))
    assert call(logits=0) == -1                                 # QL_ERR_NULL_POINTER
    assert call(row_params=0) == -1
    assert call(ldl=N - 1) == -2                                # QL_ERR_BAD_SHAPE
    assert call(out_ld=0) == -2
    assert call(stop=N) == -2
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert call(widx=rows.live.data_ptr()) == -1                # bookkeeping buffers go together
    p = torch.zeros(B, 100, device=DEV)
    assert call(probs=p.data_ptr()) == -1                       # probs without indices
    assert call(probs=p.data_ptr(), idx=rows.out_tokens.data_ptr(), dist_ld=50) == -2
    torch.cuda.synchronize()
    assert int(rows.live[0]) == B and rows.row_state.cpu().tolist() == [[0, 0]] * B     # nothing ran
    with pytest.raises(ValueError):
        fused_ops.batch_sample_advance(lg, tok[:1], rows)


def test_graph_replay_draws_fresh_numbers_and_reproduces():
    name = "vocab_default"
    _, N, _, dtype, top_k, top_p, temperature = SC.CASES[name]
    B, steps = 4, 24
    lg = torch.from_numpy(SC.logits_for(name)).to(TDT[dtype]).to(DEV)[None].expand(B, N).contiguous()
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    params = [(top_k, top_p, temperature)] * B
    seeds = [11, 12, 13, 11]                                    # rows 0 and 3: the same generator key -> the same stream
    rows = rows_of(B, steps, params, seeds, [steps] * B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused_ops.batch_sample_advance(lg, tok, rows)
    torch.cuda.current_stream().wait_stream(side)
    rows.arm(params, seeds, [steps] * B)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fused_ops.batch_sample_advance(lg, tok, rows)
    rows.arm(params, seeds, [steps] * B)
    for _ in range(steps + 3):                                  # three replays past the budget: nothing changes
        graph.replay()
    torch.cuda.synchronize()
    seen = rows.out_tokens.cpu().numpy()
    want_p, want_i = O.top_p_filter(SC.logits_for(name), top_k, top_p, temperature)
    assert int(rows.live[0]) == 0 and rows.row_state.cpu().tolist() == [[steps, 1]] * B
    assert rows.row_rng[:, 1].cpu().tolist() == [steps] * B
    assert len(set(seen[0].tolist())) > 6, "replays repeated one draw"
    assert set(seen.ravel().tolist()) <= set(want_i[want_p > 0].tolist())
    assert np.array_equal(seen[0], seen[3]) and not np.array_equal(seen[0], seen[1])
    rows.arm(params, seeds, [steps] * B)
    for _ in range(steps):
        graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(rows.out_tokens.cpu().numpy(), seen)


def test_draws_follow_the_filtered_distribution_chi_square():
    """>= 1e5 draws (1024 rows with distinct seeds x 100 launches) against the filtered probabilities: per-row keys with the row
    index outside the counter give independent streams."""
    name = "vocab_default"
    _, N, _, dtype, top_k, top_p, temperature = SC.CASES[name]
    x = SC.logits_for(name)
    want_p, want_i = O.top_p_filter(x, top_k, top_p, temperature)
    B, launches = 1024, 100
    lg = torch.from_numpy(x).to(TDT[dtype]).to(DEV)[None].expand(B, N).contiguous()
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    rows = rows_of(B, launches, [(top_k, top_p, temperature)] * B, [777 + 31 * b for b in range(B)], [launches] * B)
    for _ in range(launches):
        fused_ops.batch_sample_advance(lg, tok, rows)
    counts = torch.bincount(rows.out_tokens.view(-1), minlength=N).cpu().numpy()
    n = B * launches
    assert counts.sum() == n and int(rows.live[0]) == 0
    assert counts[np.setdiff1d(np.arange(N), want_i[want_p > 0])].sum() == 0, "a token outside the filtered support was drawn"
    obs, exp = counts[want_i].astype(np.float64), want_p.astype(np.float64) * n
    keep = exp >= 5
    chi2 = float((((obs - exp) ** 2) / np.where(keep, exp, 1))[keep].sum())
    dof = int(keep.sum()) - 1
    from scipy import stats
    assert chi2 < stats.chi2.ppf(1 - 1e-4, dof), (chi2, dof)


# ---- the session and the API --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    model, cfg = build_tiny("f16", DEV)
    return model, cfg


@pytest.fixture(scope="module")
def real16():
    model, cfg = build_real(DEV)
    return model, cfg


def prompts_of(name):
    ids, attn = Z[f"{name}/ids"], Z[f"{name}/attention_mask"]
    return [ids[b][attn[b] == 1].tolist() for b in range(ids.shape[0])]


def teacher_forced(model, prompts, tokens):
    """Every step's last-position logits (B, T, V) fp32 of the batch fed the given tokens, through an eager "logits"-mode session of
    the same batch (left padded as generate_batch_ids pads)."""
    B, S, T = len(prompts), max(len(p) for p in prompts), len(tokens[0])
    ids = torch.zeros(B, S, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    out = [sess.prefill(ids, attention_mask=attn).float()]
    tk = torch.tensor(tokens, dtype=torch.long)
    for t in range(1, T):
        out.append(sess.decode_step(tk[:, t - 1:t], greedy=False).float())
    return torch.stack(out, dim=1).cpu()


@pytest.mark.parametrize("name", ["tiny/f16", "real/b4"])
def test_greedy_batch_against_reference(name, tiny16, real16):
    model, cfg = tiny16 if name.startswith("tiny") else real16
    tol = TINY_TOL["f16"] if name.startswith("tiny") else REAL_TOL
    want, margin = Z[f"{name}/tokens"], Z[f"{name}/margin"]
    ref_logits = Z[f"{name}/logits"].astype(np.float32)
    B, T = want.shape
    prompts = prompts_of(name)
    got = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True)
    assert [len(r) for r in got] == [T] * B
    tf = teacher_forced(model, prompts, want.tolist()).numpy()
    noise = np.abs(tf - ref_logits).max(axis=-1)               # (B, T)
    # the project's logits bar, applied as test_model_gpu.py / test_model_real_gpu.py apply it: rel-L2 of the whole logits tensor
    rel = O.rel_l2(tf, ref_logits)
    per = max(O.rel_l2(tf[b, t], ref_logits[b, t]) for b in range(B) for t in range(T))
    compared = margin > 4 * noise
    print(f"[batch generate vs reference] {name}: noise max {noise.max():.3e} mean {noise.mean():.3e}, rel-L2 {rel:.3e} (bar {tol}; "
          f"worst single (row, step) {per:.3e}), compared {int(compared.sum())} of {B * T} ({compared.mean():.0%})")
    assert rel <= tol, rel
    n_cmp = 0
    for b in range(B):
        for t in range(T):
            if got[b][t] != want[b, t]:
                assert not compared[b, t], (name, b, t, got[b][t], int(want[b, t]), float(margin[b, t]), float(noise[b, t]))
                break                                           # a diverged row: its later steps are not compared
            n_cmp += int(compared[b, t])
    assert n_cmp >= 0.8 * B * T, (n_cmp, B * T)


def test_graph_equals_eager_and_sampled_tokens_recompute(tiny16):
    model, cfg = tiny16
    prompts = [[5, 9, 200, 31, 7], [44, 3], [100, 101, 102, 103, 104, 105, 106, 107], [250]]
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=10, ignore_eos=True)
    g_greedy = dec.generate_batch_ids(prompts, greedy=True, use_graph=True, **kw)
    e_greedy = dec.generate_batch_ids(prompts, greedy=True, use_graph=False, **kw)
    assert g_greedy == e_greedy
    skw = dict(kw, top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])
    g_s = dec.generate_batch_ids(prompts, use_graph=True, **skw)
    e_s = dec.generate_batch_ids(prompts, use_graph=False, **skw)
    assert g_s == e_s and dec.last_stats["generated"] == [10] * 4
    # every sampled token from the teacher-forced logits of the same batch, the oracle's distribution and Philox (seed_b, step)
    lg = teacher_forced(model, prompts, g_s).numpy()
    for b in range(4):
        k, p, t = skw["top_k"][b], skw["top_p"][b], skw["temperature"][b]
        for s in range(10):
            want_p, want_i = O.top_p_filter(lg[b, s], k, p, t)
            if k == 1:
                assert g_s[b][s] == int(np.argmax(lg[b, s]))
                continue
            u = _philox.uniform(skw["seed"][b], s, 0)
            assert inverse_cdf_ok(g_s[b][s], want_p, want_i, u), (b, s)


def test_batch_of_one_equals_generate_ids(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250, 8, 61]
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=14, ignore_eos=True)
    assert dec.generate_batch_ids([p], greedy=True, **kw) == [list(dec.generate_ids(p, greedy=True, **kw))]
    assert dec.generate_batch_ids([p], seed=31, **kw) == [list(dec.generate_ids(p, seed=31, **kw))]
    torch.manual_seed(9)
    a = dec.generate_batch_ids([p], **kw)
    torch.manual_seed(9)
    assert a == [list(dec.generate_ids(p, **kw))]               # seed None: both take theirs from torch's global generator


def test_row_permutation(tiny16):
    model, cfg = tiny16
    prompts = [[5, 9, 200, 31, 7], [44, 3], [100, 101, 102, 103, 104, 105, 106, 107], [250], [12, 13, 14]]
    seeds = [101, 202, 303, 404, 505]
    kw = dict(max_generated_tokens=9, ignore_eos=True, top_k=[100, 1, 100, 30, 100])
    base = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, seed=seeds, **kw)
    perm = [3, 0, 4, 2, 1]
    kw_p = dict(kw, top_k=[kw["top_k"][i] for i in perm])
    got = ChatGLMDecoder(cfg, model).generate_batch_ids([prompts[i] for i in perm], seed=[seeds[i] for i in perm], **kw_p)
    assert got == [base[i] for i in perm]


def test_eos_stops_a_row_and_the_loop(tiny16):
    model, cfg = tiny16
    prompts = [[5, 9, 200, 31, 7], [44, 3], [100, 101, 102, 103, 104, 105, 106, 107]]
    T = 30
    base = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=T, greedy=True, ignore_eos=True)
    pick = None
    for r in range(3):
        for j, t in enumerate(base[r]):
            if 4 <= j < T - 8 and base[r].index(t) == j and all(t not in base[o] for o in range(3) if o != r):
                pick = (r, j, t)
                break
        if pick:
            break
    assert pick is not None, base
    r, j, eos = pick
    budgets = [3] * 3
    budgets[r] = T
    poll = 2
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    got = dec.generate_batch_ids(prompts, max_generated_tokens=budgets, greedy=True, poll_every=poll)
    assert got[r] == base[r][:j + 1]
    assert all(got[o] == base[o][:3] for o in range(3) if o != r)
    last = max(len(x) for x in got) - 1                         # the step at which the last row finished
    print(f"[batch generate eos] finished at step {last}, ran {dec.last_stats['steps']} steps (poll_every {poll})")
    assert dec.last_stats["steps"] <= last + 2 * poll + 1


@pytest.mark.parametrize("B", [2, 3, 8, 17, 33])
def test_batch_sizes_across_the_dispatch_table(B, real16):
    """rows4 / rows16 / fewrow / the 32-row GEMM in the step: the graph's greedy tokens equal the teacher-forced argmax."""
    model, cfg = real16
    g = torch.Generator().manual_seed(500 + B)
    prompts = [torch.randint(1, cfg.vocab_size, (int(n),), generator=g).tolist()
               for n in torch.randint(3, 20, (B,), generator=g)]
    got = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, max_generated_tokens=6, greedy=True, ignore_eos=True)
    lg = teacher_forced(model, prompts, got)
    assert np.array_equal(lg.argmax(dim=-1).numpy(), np.array(got))


def test_mode_switching_on_one_decoder(tiny16):
    model, cfg = tiny16
    prompts = [[5, 9, 200, 31, 7], [44, 3], [100, 101, 102]]
    p = [17, 3, 99, 250]
    bkw = dict(max_generated_tokens=8, ignore_eos=True, seed=[1, 2, 3])
    gkw = dict(max_generated_tokens=8, ignore_eos=True)

    def host_sampled(d):
        torch.manual_seed(21)
        return list(d.generate_ids(p, device_sampler=False, **gkw))
    fresh = ChatGLMDecoder(cfg, model)
    want = (fresh.generate_batch_ids(prompts, **bkw), list(ChatGLMDecoder(cfg, model).generate_ids(p, greedy=True, **gkw)),
            host_sampled(ChatGLMDecoder(cfg, model)))
    dec = ChatGLMDecoder(cfg, model)
    assert dec.generate_batch_ids(prompts, **bkw) == want[0]
    assert list(dec.generate_ids(p, greedy=True, **gkw)) == want[1]
    assert host_sampled(dec) == want[2]
    assert dec.generate_batch_ids(prompts, **bkw) == want[0]
    sess = dec._batch_sessions[3][1]
    assert "rows" in sess._graphs


def test_low_footprint_gives_the_same_tokens(tiny16):
    model, cfg = tiny16
    prompts = [[5, 9, 200, 31, 7], [44, 3], [100, 101, 102]]
    kw = dict(max_generated_tokens=8, ignore_eos=True, seed=[4, 5, 6])
    want = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, **kw)
    lf_model, _ = build_tiny("f16", DEV)
    got = ChatGLMDecoder(cfg, lf_model, low_footprint=True).generate_batch_ids(prompts, **kw)
    assert got == want

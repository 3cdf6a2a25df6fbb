"""Log-probabilities during generation on the GPU: ``qlinear_step_logprobs`` (csrc/logprob.hip) through ``fused_ops`` / ctypes
against ``qlinear_token_logprob`` - the float64-validated scoring kernel, bit for bit - and the float64 oracle's order
(tests/_logprobs_oracle.py), and the "+lp" steps of ``DecodeSession`` / ``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids``
against a teacher-forced eager loop written there, against themselves (graph / eager, device loop, batch of one, row permutations,
mode switches) and against the launch counter."""
import numpy as np
import pytest
import torch

import _logprobs_oracle as LO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny
from test_model_real_cpu import build_real

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
NTOPS = (0, 1, 5, 20)
R_ALL = 32
SENTINEL = -7


def make_rows(dt, N):
    """R_ALL rows of N logits: the adversarial rows first, then rows seeded at scales 1 / 4 / 12."""
    g = torch.Generator().manual_seed(7000 + N)
    x = torch.randn(R_ALL, N, generator=g) * torch.tensor([1.0, 4.0, 12.0]).repeat(R_ALL)[:R_ALL, None]
    x[0] = 1.25                                                  # constant: ids 0 .. n-1
    x[1] = torch.sort(x[1])[0]                                   # ascending
    x[2] = torch.sort(x[2], descending=True)[0]                  # descending
    x[3] = NINF                                                  # -inf but for three entries
    for i, v in zip((N // 2, N - 1, min(1, N - 1)), (0.5, -2.0, 3.0)):
        x[3, i] = v
    # equal values straddling the cut at ranks 1, 5 and 20: ranks (0, 1), (4, 5), (19, 20) are tied pairs, the lower index wins
    k = min(N, 25)
    spots = torch.randperm(N, generator=g)[:k]
    vals = 50.0 - torch.arange(k, dtype=torch.float32)
    for a in (0, 4, 19):
        if a + 1 < k:
            vals[a + 1] = vals[a]
    x[4] = torch.randn(N, generator=g)
    x[4, spots] = vals
    x[5] = torch.randn(N, generator=g) * 4
    x[5, N // 3] = 60000.0
    x[6] = torch.randn(N, generator=g)                           # one value 4096 times above everything else: the slow path
    x[6, torch.randperm(N, generator=g)[:min(4096, max(1, N // 2))]] = 9.5
    return x.to(TDT[dt])


_CASES = {}


def case(dt, N):
    """Rows, the oracle's order (R_ALL, 20) padded with -1, the chosen ids - computed once per (dtype, N), never modified."""
    if (dt, N) not in _CASES:
        x = make_rows(dt, N)
        host = x.double().numpy()
        ids = np.stack([LO.top(host[r], 20)[0] for r in range(R_ALL)])
        tok = torch.tensor([int(ids[r, min(r % 4, N - 1)]) for r in range(R_ALL)], dtype=torch.int64)
        tok[9] = N                                               # outside the vocabulary: NaN
        tok[10] = -1
        _CASES[(dt, N)] = (x, ids, tok)
    return _CASES[(dt, N)]


def reference(view, ids, tok):
    """``token_logprob`` of every row of the device tensor at the chosen id and at each of the 20 ordered ids (-1: -inf)."""
    dev = view.device
    chosen = fused_ops.token_logprob(view, tok.to(dev)).cpu()
    cols = []
    for j in range(20):
        tj = torch.from_numpy(ids[:, j]).to(dev)
        lp = fused_ops.token_logprob(view, tj.clamp(min=0)).cpu()
        cols.append(torch.where(torch.from_numpy(ids[:, j]) < 0, torch.full_like(lp, NINF), lp))
    return chosen, torch.stack(cols, dim=1)


@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("N", [1, 7, 8, 1000, 1024, 65024, 65025])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_kernel_equals_token_logprob_and_the_oracle_order(dt, N, B):
    x, ids, tok = case(dt, N)
    R = 32 if B == 32 else 12
    cap = 3
    pad = torch.full((R_ALL, N + 3), float("nan"), dtype=TDT[dt])
    pad[:, :N] = x
    for layout, view in (("contiguous", x.to(DEV)), ("ldl = N + 3, NaN pads", pad.to(DEV)[:, :N])):
        want_c, want_t = reference(view, ids, tok)
        for n_top in NTOPS:
            before = _lib.launch_count()
            for r0 in range(0, R, B):
                st = fused_ops.StepLogprobs(B, cap, DEV, n_top=n_top)
                for t in st.tensors()[1:]:
                    t.fill_(SENTINEL)
                c0 = torch.tensor([(r0 + b) % cap for b in range(B)], dtype=torch.int32)
                st.count.copy_(c0)
                fused_ops.step_logprobs(view[r0:r0 + B], tok[r0:r0 + B].to(DEV), st)
                count, chosen, top_ids, top_lp = st.fetch()
                assert torch.equal(count, c0 + 1), (layout, n_top, r0)
                for b in range(B):
                    r, c = r0 + b, int(c0[b])
                    tag = (dt, N, B, layout, n_top, r)
                    assert torch.allclose(chosen[b, c], want_c[r], rtol=0, atol=0, equal_nan=True), (tag, chosen[b, c], want_c[r])
                    assert top_ids[b, c].tolist() == ids[r, :n_top].tolist(), (tag, top_ids[b, c].tolist(), ids[r, :n_top].tolist())
                    assert torch.allclose(top_lp[b, c], want_t[r, :n_top], rtol=0, atol=0, equal_nan=True), (tag, top_lp[b, c], want_t[r, :n_top])
                    # nothing outside slot c of the row's buffers changed
                    chosen[b, c] = SENTINEL
                    top_ids[b, c] = SENTINEL
                    top_lp[b, c] = SENTINEL
                assert bool((chosen == SENTINEL).all()) and bool((top_ids == SENTINEL).all()) and bool((top_lp == SENTINEL).all())
            assert _lib.launch_count() == before + R // B, "the rows did not go through libqlinear_hip.so"
    assert ids[0, :min(N, 20)].tolist() == list(range(min(N, 20)))              # the constant row


def test_skip_rule_and_full_rule():
    B, N, cap = 5, 1000, 4
    x = (torch.randn(B, N, generator=torch.Generator().manual_seed(2)) * 4).half().to(DEV)
    tok = torch.tensor([1, 2, 3, 4, 5], dtype=torch.int64, device=DEV)
    st = fused_ops.StepLogprobs(B, cap, DEV, n_top=5)
    for t in st.tensors()[1:]:
        t.fill_(SENTINEL)
    c0 = [0, 2, 1, 4, 3]
    st.count.copy_(torch.tensor(c0, dtype=torch.int32))
    # row 0 live; row 1 finished (flag set, 2 tokens, 2 recorded); row 2 live; row 3 live but the record is full (count == cap);
    # row 4 out of budget: its token count equals its recorded entries
    row_state = torch.tensor([[1, 0], [2, 1], [2, 0], [5, 0], [3, 0]], dtype=torch.int32, device=DEV)
    before = st.fetch()
    fused_ops.step_logprobs(x, tok, st, row_state)
    after = st.fetch()
    assert after[0].tolist() == [1, 2, 2, 4, 3]
    want = fused_ops.token_logprob(x, tok).cpu()
    for b in (1, 3, 4):                                          # untouched rows: byte-identical
        assert all(torch.equal(a[b], z[b]) for a, z in zip(after, before))
    for b in (0, 2):
        assert float(after[1][b, c0[b]]) == float(want[b])
        assert after[2][b, c0[b]].tolist() == LO.order(x[b].float().cpu().numpy())[:5].tolist()
        for t in after[1:]:
            t[b, c0[b]] = SENTINEL
        assert all(torch.equal(a[b], z[b]) for a, z in zip(after[1:], before[1:]))
    # the full rule alone, through the C entry point: status 0, nothing moves
    lib = _lib.get_lib()
    st.count.fill_(cap)
    before = st.fetch()
    status = lib.qlinear_step_logprobs(x.data_ptr(), B, N, N, tok.data_ptr(), None, st.count.data_ptr(), st.chosen.data_ptr(),
                                       st.top_ids.data_ptr(), st.top_lp.data_ptr(), cap, 5, _lib.dtype_code(x.dtype), _lib.stream_ptr(x.device))
    assert status == 0
    assert all(torch.equal(a, z) for a, z in zip(st.fetch(), before))


def test_argument_errors_return_status_codes():
    lib = _lib.get_lib()
    B, N, cap = 2, 100, 4
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    st = fused_ops.StepLogprobs(B, cap, DEV)
    f16 = _lib.dtype_code(torch.float16)

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, tk=tok.data_ptr(), count=st.count.data_ptr(), chosen=st.chosen.data_ptr(),
             ids=st.top_ids.data_ptr(), lps=st.top_lp.data_ptr(), cp=cap, n_top=20, dtype=f16):
        return lib.qlinear_step_logprobs(logits, b, n, ldl, tk, None, count, chosen, ids, lps, cp, n_top, dtype, _lib.stream_ptr(lg.device))
    before = _lib.launch_count()
    assert call(logits=0) == -1                                 # QL_ERR_NULL_POINTER
    assert call(tk=0) == -1
    assert call(count=0) == -1
    assert call(chosen=0) == -1
    assert call(ids=0) == -1 and call(lps=0) == -1              # alternatives are asked for (n_top > 0) but a buffer is missing
    assert call(n=0) == -2                                      # QL_ERR_BAD_SHAPE
    assert call(ldl=N - 1) == -2
    assert call(b=65536) == -2
    assert call(cp=0) == -2
    assert call(n_top=21) == -2 and call(n_top=-1) == -2
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(logits=lg.data_ptr() + 1) == -5                 # QL_ERR_MISALIGNED, as qlinear_token_logprob
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert _lib.launch_count() == before
    torch.cuda.synchronize()
    assert int(st.count.sum()) == 0                             # nothing ran
    assert call(ids=0, lps=0, n_top=0) == 0 and _lib.launch_count() == before + 1       # no alternatives: the buffers may be null
    torch.cuda.synchronize()
    assert st.count.tolist() == [1, 1]
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(lg[:1], tok[:1], st)
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(lg, tok.int(), st)
    with pytest.raises(ValueError):
        fused_ops.step_logprobs(lg, tok.cpu(), st)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_nan_logit_stays_in_its_row(dt):
    B, N = 3, 65024
    x = (torch.randn(B, N, generator=torch.Generator().manual_seed(4)) * 4).to(TDT[dt])
    x[1, 40000] = float("nan")
    xd = x.to(DEV)
    tok = torch.tensor([5, 6, 7], dtype=torch.int64, device=DEV)
    st = fused_ops.StepLogprobs(B, 2, DEV, n_top=5)
    fused_ops.step_logprobs(xd, tok, st)
    _, chosen, ids, lps = st.fetch()
    assert bool(torch.isnan(chosen[1, 0])) and bool(torch.isnan(lps[1, 0]).all())
    assert ids[1, 0].tolist() == LO.order(x[1].float().numpy())[:5].tolist()    # the NaN ranks last: the order is that of the numbers
    want = fused_ops.token_logprob(xd, tok).cpu()
    for b in (0, 2):
        assert float(chosen[b, 0]) == float(want[b]) and bool(torch.isfinite(lps[b, 0]).all())
        assert ids[b, 0].tolist() == LO.order(x[b].float().numpy())[:5].tolist()


# ---- the session and the API --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


@pytest.fixture(scope="module")
def real16():
    return build_real(DEV)


PROMPTS = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0], [250]]
PEN = dict(repetition_penalty=[1.5, 1.0, 1.2, 0.8], presence_penalty=[0.0, 0.7, 0.0, -0.2], frequency_penalty=[0.4, 0.0, 0.1, 0.05])
ROWS = dict(top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])


def flat(rec):
    return (rec.token_logprobs, rec.top_ids, rec.top_logprobs)


@pytest.mark.parametrize("name", ["tiny", "real"])
def test_generate_ids_logprobs_equal_the_loop(name, tiny16, real16):
    model, cfg = tiny16 if name == "tiny" else real16
    p = [17, 3, 99, 250, 8, 61]
    T = 10
    dec = ChatGLMDecoder(cfg, model)
    for mode in (dict(greedy=True), dict(seed=77)):
        kw = dict(max_generated_tokens=T, ignore_eos=True, **mode)
        base = list(dec.generate_ids(p, **kw))
        assert dec.last_logprobs is None and dec.last_stats["logprobs"] is False
        got = list(dec.generate_ids(p, logprobs=5, **kw))
        rec = dec.last_logprobs
        assert got == base and dec.last_stats["logprobs"] is True and len(rec) == T
        assert ("greedy+lp" if "greedy" in mode else "sample+lp") in dec._session._graphs
        if "greedy" in mode:
            assert all(rec.top_ids[t][0] == got[t] for t in range(T))
        LO.check_record(LO.replay_logits(model, [p], [got]), [got], [rec], 5)
        # eager steps, the device loop (no per-token read-back), fewer alternatives: the same record
        assert list(dec.generate_ids(p, logprobs=5, use_graph=False, **kw)) == got and flat(dec.last_logprobs) == flat(rec)
        assert list(dec.generate_ids(p, logprobs=5, sync_every_token=False, **kw)) == got and flat(dec.last_logprobs) == flat(rec)
        assert list(dec.generate_ids(p, logprobs=2, **kw)) == got
        assert dec.last_logprobs.token_logprobs == rec.token_logprobs and dec.last_logprobs.top_ids == [r[:2] for r in rec.top_ids]
    # the host-decides path (device_sampler=False) with penalties: the record is that of the logits the host sampled from
    pen = dict(repetition_penalty=1.3, presence_penalty=0.2, logit_bias={base[0]: NINF})
    torch.manual_seed(9)
    plain = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, device_sampler=False, **pen))
    torch.manual_seed(9)
    got = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, device_sampler=False, logprobs=3, **pen))
    assert got == plain
    LO.check_record(LO.replay_logits(model, [p], [got], [(1.3, 0.2, 0.0)], [pen["logit_bias"]]), [got], [dec.last_logprobs], 3)
    # penalised greedy on the captured step: the launch order (penalties, selection, record)
    got = list(dec.generate_ids(p, max_generated_tokens=T, ignore_eos=True, greedy=True, logprobs=3, **pen))
    assert "greedy+pen+lp" in dec._session._graphs
    LO.check_record(LO.replay_logits(model, [p], [got], [(1.3, 0.2, 0.0)], [pen["logit_bias"]]), [got], [dec.last_logprobs], 3)


@pytest.mark.parametrize("name", ["tiny", "real"])
def test_generate_batch_ids_logprobs_equal_the_loop(name, tiny16, real16):
    model, cfg = tiny16 if name == "tiny" else real16
    budgets = [9, 2, 9, 9]
    dec = ChatGLMDecoder(cfg, model)
    first = dec.generate_batch_ids(PROMPTS, max_generated_tokens=budgets, greedy=True, ignore_eos=True)
    bias = [None, {first[1][0]: -1.0}, {first[2][0]: NINF}, {first[3][1]: NINF, 7: 0.5}]
    kw = dict(max_generated_tokens=budgets, ignore_eos=True, logit_bias=bias, **PEN, **ROWS)
    base = dec.generate_batch_ids(PROMPTS, **kw)
    assert dec.last_logprobs is None
    got = dec.generate_batch_ids(PROMPTS, logprobs=5, **kw)
    recs = dec.last_logprobs
    assert got == base and [len(g) for g in got] == budgets and [len(r) for r in recs] == budgets
    assert "rows+pen+lp" in dec._batch_sessions[4][1]._graphs and dec.last_stats["logprobs"] is True
    settings = list(zip(*(PEN[k] for k in ("repetition_penalty", "presence_penalty", "frequency_penalty"))))
    LO.check_record(LO.replay_logits(model, PROMPTS, got, settings, bias), got, recs, 5)
    assert all(recs[3].top_ids[t][0] == got[3][t] for t in range(budgets[3]))   # row 3 is a top_k 1 row
    # eager steps give the same record
    assert dec.generate_batch_ids(PROMPTS, logprobs=5, use_graph=False, **kw) == got
    assert [flat(r) for r in dec.last_logprobs] == [flat(r) for r in recs]
    # without penalties: "rows+lp"
    plain = {k: v for k, v in kw.items() if k not in PEN and k != "logit_bias"}
    got = dec.generate_batch_ids(PROMPTS, logprobs=1, **plain)
    assert "rows+lp" in dec._batch_sessions[4][1]._graphs
    LO.check_record(LO.replay_logits(model, PROMPTS, got), got, dec.last_logprobs, 1)


def test_batch_of_one_and_row_permutation(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250, 8, 61]
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=12, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.2, logit_bias={3: NINF}, logprobs=4)
    for mode in (dict(seed=31), dict(greedy=True)):
        batch = dec.generate_batch_ids([p], **mode, **kw)
        one_rec = dec.last_logprobs[0]
        assert batch == [list(dec.generate_ids(p, **mode, **kw))] and flat(dec.last_logprobs) == flat(one_rec)
    prompts = PROMPTS + [[12, 13, 14]]
    args = dict(seed=[101, 202, 303, 404, 505], top_k=[100, 1, 100, 30, 100], repetition_penalty=[1.5, 1.0, 1.2, 0.8, 1.0],
                max_generated_tokens=[9, 2, 9, 5, 9])
    d0 = ChatGLMDecoder(cfg, model)
    base = d0.generate_batch_ids(prompts, ignore_eos=True, logprobs=3, **args)
    base_recs = d0.last_logprobs
    perm = [3, 0, 4, 2, 1]
    pick = lambda v: [v[i] for i in perm]
    d1 = ChatGLMDecoder(cfg, model)
    got = d1.generate_batch_ids(pick(prompts), ignore_eos=True, logprobs=3, **{k: pick(v) for k, v in args.items()})
    assert got == pick(base)
    assert [flat(r) for r in d1.last_logprobs] == [flat(r) for r in pick(base_recs)]


def test_a_run_that_ends_on_the_end_token(tiny16):
    """The greedy ahead-launch has launched the step behind the end token before the host reads it: that step's entry is in the
    device record and must not reach the result."""
    model, cfg = tiny16
    p = [17, 3, 99, 250, 8, 61]
    base = list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=12, greedy=True, ignore_eos=True))
    k = max(base.index(t) for t in base)                        # the id whose first appearance comes last ends the run there
    assert k >= 1
    dec = ChatGLMDecoder(cfg, model, eos_token_id=base[k])
    got = list(dec.generate_ids(p, max_generated_tokens=12, greedy=True, logprobs=2))
    rec = dec.last_logprobs
    assert got == base[:k + 1] and len(rec) == len(got)
    torch.cuda.synchronize()
    recorded = int(dec._session.lp.count[0])
    print(f"[end token] {len(got)} tokens returned, {recorded} entries recorded on the device")
    assert recorded >= len(got)
    LO.check_record(LO.replay_logits(model, [p], [got]), [got], [rec], 2)
    # the batch loop runs past its last row's end: finished rows record nothing
    bdec = ChatGLMDecoder(cfg, model, eos_token_id=base[k])
    out = bdec.generate_batch_ids([p, p[:3]], max_generated_tokens=12, greedy=True, logprobs=2)
    assert [len(r) for r in bdec.last_logprobs] == [len(o) for o in out] and bdec.last_stats["steps"] >= max(len(o) for o in out) - 1
    assert bdec._batch_sessions[2][1].lp.count.tolist() == [len(o) for o in out]


def test_capture_records_nothing(tiny16):
    model, cfg = tiny16
    B, n = 3, 7
    prompts = [[5, 9, 200], [44, 3, 1], [100, 101, 102]]
    for mode in ("rows", "greedy", "sample"):
        sess = DecodeSession(model, B, 64, use_graph=True)
        assert sess.lp is None
        assert sess.arm_logprobs(True) and sess.lp is not None
        sess.arm_rows([(1, 0.8, 1.0)] * B, [1, 2, 3], [2, n + 5, n + 5])            # row 0 stops after two tokens
        sess.set_sampling(50, 0.9, 1.0, seed=3)
        logits = sess.prefill(torch.tensor(prompts))
        if mode == "rows":
            sess.sample_rows_first(logits)
        elif mode == "sample":
            sess.sample_first(logits)
        else:
            sess.tok.copy_(logits.argmax(-1, keepdim=True))
        kw = dict(greedy=mode == "greedy", sample=mode == "sample", rows=mode == "rows", lp=True)
        sess.capture(**kw)
        torch.cuda.synchronize()
        assert sess.lp.count.tolist() == [0] * B, "the capture's warm-up runs recorded entries"
        sess.logprobs_first(logits, rows=mode == "rows")
        for _ in range(n):
            sess.decode_step(**kw)
        torch.cuda.synchronize()
        assert mode + "+lp" in sess._graphs
        assert sess.lp.count.tolist() == ([2, n + 1, n + 1] if mode == "rows" else [n + 1] * B)
    with pytest.raises(RuntimeError):
        DecodeSession(model, B, 64, use_graph=True).capture(greedy=True, lp=True)


def test_launch_accounting(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250]
    T = 9

    def launches(fn):
        before = _lib.launch_count()
        fn()
        torch.cuda.synchronize()
        return _lib.launch_count() - before

    warm = ChatGLMDecoder(cfg, model)                            # build every lazy layout the steps read before anything is counted
    list(warm.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    warm.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    # eager steps: a recorded token costs exactly one launch more (T - 1 steps and the first token)
    for gen in (lambda d, **k: list(d.generate_ids(p, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k)),
                lambda d, **k: d.generate_batch_ids(PROMPTS, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k)):
        for mode in (dict(greedy=True), dict(seed=3)):
            off = launches(lambda: gen(ChatGLMDecoder(cfg, model), **mode))
            on = launches(lambda: gen(ChatGLMDecoder(cfg, model), **mode, logprobs=0))
            assert on == off + T, (on, off, mode)
    # graphs: a plain generation on a session that holds "+lp" graphs issues what it issues on a fresh session
    fresh = launches(lambda: list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    dec = ChatGLMDecoder(cfg, model)
    list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, logprobs=5))
    assert launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))) == fresh
    assert set(dec._session._graphs) == {"greedy+lp", "greedy"}
    # ... and replays: a recorded generation issues one launch more than the plain one - the first token's
    again = launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    lp_again = launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, logprobs=5)))
    assert lp_again == again + 1
    bdec = ChatGLMDecoder(cfg, model)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, logprobs=5)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True)
    again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    lp_again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, logprobs=5))
    assert lp_again == again + 1


def test_mode_switching_on_one_session(tiny16):
    """plain -> "+lp" -> "+pen+lp" -> plain on ONE reused session: each run gives the tokens of a fresh decoder."""
    model, cfg = tiny16
    p = [17, 3, 99, 250]
    kw = dict(max_generated_tokens=10, ignore_eos=True)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2, logit_bias={5: NINF})
    fresh = lambda **k: list(ChatGLMDecoder(cfg, model).generate_ids(p, **kw, **k))
    dec = ChatGLMDecoder(cfg, model)
    for mode in (dict(greedy=True), dict(seed=21)):
        plain = list(dec.generate_ids(p, **kw, **mode))
        sess = dec._session
        assert list(dec.generate_ids(p, logprobs=5, **kw, **mode)) == plain == fresh(**mode)
        rec = dec.last_logprobs
        pen_lp = list(dec.generate_ids(p, logprobs=5, **kw, **mode, **pen))
        assert pen_lp == fresh(**mode, **pen) and 5 not in pen_lp
        assert list(dec.generate_ids(p, **kw, **mode)) == plain and dec.last_logprobs is None
        assert list(dec.generate_ids(p, logprobs=5, **kw, **mode)) == plain and flat(dec.last_logprobs) == flat(rec)
        assert dec._session is sess
    assert {"greedy", "greedy+lp", "greedy+pen+lp", "sample", "sample+lp", "sample+pen+lp"} <= set(sess._graphs)
    # a different stop id drops every captured "rows..." step, the recorded ones included
    bdec = ChatGLMDecoder(cfg, model, eos_token_id=3)
    a = bdec.generate_batch_ids(PROMPTS, max_generated_tokens=6, greedy=True, logprobs=1)
    bsess = bdec._batch_sessions[4][1]
    assert "rows+lp" in bsess._graphs
    bdec.eos_token_id = 4
    b = bdec.generate_batch_ids(PROMPTS, max_generated_tokens=6, greedy=True, logprobs=1)
    assert bsess._rows_stop == 4 and "rows+lp" in bsess._graphs
    want = ChatGLMDecoder(cfg, model, eos_token_id=4).generate_batch_ids(PROMPTS, max_generated_tokens=6, greedy=True)
    assert b == want and [len(r) for r in bdec.last_logprobs] == [len(o) for o in b] and len(a) == len(b)

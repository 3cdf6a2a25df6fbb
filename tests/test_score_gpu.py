"""Scoring on the session path on the GPU, all through the C ABI: the one-pass log-prob kernel (``qlinear_token_logprob``)
against float64 on the same logits, ``DecodeSession.score`` against its own logits, against the REFERENCE model's
``forward(labels=...)`` (tests/golden/score.npz, generator: tests/golden/make_golden_score.py), its footprint and the state it
leaves behind.  Measured values are printed (pytest -s) and recorded in DESIGN.md section 6."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _golden as G  # noqa: E402
from oracle import qlinear_oracle as O  # noqa: E402
from chatglm_q_amd import _lib, fused_ops  # noqa: E402
from chatglm_q_amd import model as M  # noqa: E402
from chatglm_q_amd.decoder import DecodeSession  # noqa: E402
from test_model_cpu import build as build_tiny  # noqa: E402
from test_model_real_cpu import build_real  # noqa: E402

DEV = "cuda:0"
Z = G.load("score.npz")
# log-probs and loss against the reference model: the project's bar for logits against the reference at this width
# (tests/test_model_real_gpu.py: TOL), applied to the quantity derived from them
TOL = 2e-3
# the kernel against float64: FACTOR x what torch's CPU fp32 F.cross_entropy (the reference's arithmetic) measures on the same rows
FACTOR = 4.0
TDT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def case(name):
    return {k: torch.from_numpy(Z[f"{name}/{k}"]) for k in ("ids", "attention_mask", "labels", "logprobs")}, float(Z[f"{name}/loss"])


def metric(got, want):
    """max |got - want| / max(1, |want|) over the entries where `want` is finite; the others must agree exactly (inf) or both be NaN."""
    got, want = got.double().cpu(), want.double().cpu()
    fin = torch.isfinite(want)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), "infinite entries"
    if not bool(fin.any()):
        return 0.0
    return float(((got[fin] - want[fin]).abs() / want[fin].abs().clamp(min=1.0)).max())


def dense64(x, t):
    """(log-prob, lse) in float64 from logits x (R, N) (any float dtype, CPU) and targets: 0 at -100, NaN outside [0, N)."""
    xd = x.double()
    lse = torch.logsumexp(xd, dim=-1)
    N = x.shape[1]
    inside = (t >= 0) & (t < N)
    picked = xd.gather(1, t.clamp(0, N - 1)[:, None])[:, 0] - lse
    lp = torch.where(t == -100, torch.zeros_like(picked), torch.where(inside, picked, torch.full_like(picked, float("nan"))))
    return lp, lse


def reference_fp32(x, t):
    """The reference's arithmetic on the same rows: logits .float(), then F.cross_entropy (CPU, fp32), in the layout of dense64."""
    xf = x.float()
    N = x.shape[1]
    inside = (t >= 0) & (t < N)
    lp = -F.cross_entropy(xf, t.clamp(0, N - 1), reduction="none")
    lp = torch.where(t == -100, torch.zeros_like(lp), torch.where(inside, lp, torch.full_like(lp, float("nan"))))
    return lp, torch.logsumexp(xf, dim=-1)


def make_rows(R, N, dtype, seed):
    """Seeded rows at scales 1 / 4 / 12 with, where they fit, a constant row, a row holding 60000, rows of -inf with one finite
    entry, a tie of two maxima, an ignored target and out-of-range targets."""
    g = torch.Generator().manual_seed(seed)
    scale = torch.tensor([1.0, 4.0, 12.0])[torch.arange(R) % 3][:, None]
    x = (torch.randn(R, N, generator=g) * scale).to(dtype)
    t = torch.randint(0, N, (R,), generator=g)
    if R >= 5:
        x[1] = 0.75                                              # constant row: every index is a maximum, argmax 0
        x[2, N // 3] = 60000.0
        x[3] = float("-inf")
        x[3, N - 1] = -2.5                                        # one finite entry ...
        t[3] = N - 1                                              # ... is the target: log-prob 0
        t[0] = -100
        t[4] = N                                                  # just past the row
    if R >= 64:
        x[5] = float("-inf")
        x[5, N // 2] = 3.0
        t[5] = 0                                                  # a -inf entry (N > 1): log-prob -inf
        t[6] = -7
        t[8] = 2 ** 40
        if N >= 8:
            x[7, 5] = x[7, 2] = 100.0                             # two equal maxima: the lower index wins
        t[9] = -100
    return x, t


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("N", [1, 7, 8, 1000, 1024, 65024, 65025])
def test_kernel_against_float64_on_the_same_logits(N, dt):
    dtype = TDT[dt]
    worst = {"lp": 0.0, "lse": 0.0, "lp_ref": 0.0, "lse_ref": 0.0}
    before = _lib.launch_count()
    for R in (1, 5, 64, 2048):
        x, t = make_rows(R, N, dtype, 1000 * N + R)
        lp64, lse64 = dense64(x, t)
        lp32, lse32 = reference_fp32(x, t)
        worst["lp_ref"] = max(worst["lp_ref"], metric(lp32, lp64))
        worst["lse_ref"] = max(worst["lse_ref"], metric(lse32, lse64))
        first_max = torch.from_numpy(np.argmax(x.float().numpy(), axis=1))      # numpy: the first of equal maxima
        for pad in (0, 3):                                       # contiguous rows; ldl = N + 3: rows at every 2- / 4-byte alignment
            buf = torch.full((R, N + pad), float("nan"), dtype=dtype)           # a read past a row's end would poison the sum
            buf[:, :N] = x
            xg = buf.to(DEV)[:, :N]
            assert xg.stride(0) == N + pad
            lp, lse, am = fused_ops.token_logprob(xg, t.to(DEV), return_lse=True, return_argmax=True)
            worst["lp"] = max(worst["lp"], metric(lp, lp64))
            worst["lse"] = max(worst["lse"], metric(lse, lse64))
            assert torch.equal(am.cpu(), first_max), (R, N, pad)
            only = fused_ops.token_logprob(xg, t.to(DEV))        # nullable outputs
            assert torch.allclose(only, lp, rtol=0, atol=0, equal_nan=True)
    assert _lib.launch_count() >= before + 16, "the rows did not go through libqlinear_hip.so"
    print(f"[token_logprob] N={N} {dt}: log-prob err {worst['lp']:.3e} (fp32 cross_entropy: {worst['lp_ref']:.3e}), "
          f"lse err {worst['lse']:.3e} (fp32 logsumexp: {worst['lse_ref']:.3e})")
    assert worst["lp"] <= FACTOR * worst["lp_ref"]
    assert worst["lse"] <= FACTOR * worst["lse_ref"]


def test_kernel_nan_logit_stays_in_its_row_and_bad_arguments():
    x = torch.randn(4, 1000).half()
    x[2, 17] = float("nan")
    t = torch.tensor([3, 4, 5, 6])
    lp, lse = fused_ops.token_logprob(x.to(DEV), t.to(DEV), return_lse=True)
    assert bool(torch.isnan(lp[2])) and bool(torch.isnan(lse[2]))
    keep = torch.tensor([0, 1, 3])
    assert bool(torch.isfinite(lp[keep]).all()) and bool(torch.isfinite(lse[keep]).all())
    assert fused_ops.token_logprob(torch.zeros(0, 8, device=DEV), torch.zeros(0, dtype=torch.long, device=DEV)).shape == (0,)
    with pytest.raises(ValueError):
        fused_ops.token_logprob(x.to(DEV), t)                    # targets on another device
    with pytest.raises(TypeError):
        fused_ops.token_logprob(torch.zeros(2, 8, device=DEV, dtype=torch.float64), torch.zeros(2, dtype=torch.long, device=DEV))
    lib = _lib.get_lib()
    xg, tg, out = x.to(DEV), t.to(DEV), torch.zeros(4, device=DEV)
    assert lib.qlinear_token_logprob(xg.data_ptr(), 4, 1000, 999, tg.data_ptr(), -100, out.data_ptr(), None, None, 1, None) == -2
    assert lib.qlinear_token_logprob(xg.data_ptr(), 4, 1000, 1000, None, -100, out.data_ptr(), None, None, 1, None) == -1
    assert lib.qlinear_token_logprob(xg.data_ptr() + 1, 4, 1000, 1000, tg.data_ptr(), -100, out.data_ptr(), None, None, 1, None) == -5


# ---- score() -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_gpu():
    return build_real(DEV)


@pytest.fixture(scope="module")
def v65k_gpu():
    cfg = M.ChatGLM2Config(**dict(G.REAL_DIM_CONFIG, vocab_size=65024))
    model = M.create_quant_int4_model(cfg, dtype=torch.float16)
    G.fill_seeded_(model.state_dict(), int(Z["seed"][0]))
    for m in model.modules():
        if hasattr(m, "invalidate"):
            m.invalidate()
    return model.to(DEV).eval(), cfg


def own_logits(model, ids, attn, capacity):
    """All-position logits of the session route in one pass: step(last_only=False) with prefill's masks and positions."""
    B, S = ids.shape
    ids, valid = ids.to(DEV), attn.to(DEV).bool()
    positions = torch.where(valid, torch.cumsum(valid.long(), 1), torch.zeros_like(ids))
    pad_cols = torch.zeros(B, capacity, dtype=torch.bool, device=DEV)
    pad_cols[:, :S] = ~valid
    t = torch.arange(capacity, device=DEV)
    rows = torch.arange(S, device=DEV)
    mask = ((t[None, None, :] > rows[None, :, None]) | pad_cols[:, None, :]).float() * -1e10
    with torch.no_grad():
        return model.step(ids, model.new_cache(B, capacity), rows, positions, mask, last_only=False, kv_len=S)


def check_against_own_logits(tag, res, logits, labels):
    """score()'s log-probs against the dense fp32 formula's float64 restatement on the logits it was computed from, at the
    kernel's bar: FACTOR x the error of fp32 F.cross_entropy on the same rows."""
    B, S, V = logits.shape
    x = logits[:, :-1].reshape(-1, V).cpu()
    t = labels[:, 1:].reshape(-1)
    lp64, _ = dense64(x, t)
    lp32, _ = reference_fp32(x, t)
    e, e_ref = metric(res.logprobs.reshape(-1), lp64), metric(lp32, lp64)
    print(f"[score vs own logits] {tag}: err {e:.3e} (fp32 cross_entropy on the same logits: {e_ref:.3e})")
    assert e <= FACTOR * e_ref
    want_loss = -(lp64.sum() / (t != -100).sum())
    assert abs(float(res.loss) - float(want_loss)) <= 1e-5 * abs(float(want_loss))


def blockwise_logits(model, sess_like, ids, attn, chunk, head_rows, capacity):
    """The logits score(chunk, head_rows) itself forms: the same chunks through step(return_hidden=True), the same row blocks
    through head() - lm_head on 7 rows runs another kernel than on 160, its logits differ in the last fp16 bit, and the bar of
    the kernel test only means something on the logits the kernel was given."""
    B, S = ids.shape
    sess = DecodeSession(model, B, capacity, use_graph=False)
    out = torch.empty(B, S, model.config.vocab_size, dtype=sess_like.dtype, device=DEV)

    def per_chunk(s0, s1, hidden):
        h2 = hidden.reshape(B * (s1 - s0), -1)
        blocks = [model.head(h2[r0:r0 + head_rows]) for r0 in range(0, h2.shape[0], head_rows)]
        out[:, s0:s1] = torch.cat(blocks).view(B, s1 - s0, -1)

    with torch.no_grad():
        sess._prefill(ids, chunk, attn, per_chunk)
    return out


def test_score_against_its_own_logits(real_gpu):
    model, cfg = real_gpu
    c, _ = case("real/b4")
    B, S = c["ids"].shape
    sess = DecodeSession(model, B, 64, use_graph=False)
    before = _lib.launch_count()
    res = sess.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], return_argmax=True)
    assert _lib.launch_count() > before
    logits = own_logits(model, c["ids"], c["attention_mask"], 64)
    check_against_own_logits("real/b4 one pass", res, logits, c["labels"])
    assert np.array_equal(res.argmax.cpu().numpy(), np.argmax(logits[:, :-1].float().cpu().numpy(), axis=-1))   # numpy: first of equal maxima
    # row blocks and chunks that split the rows unevenly: 40 positions in chunks of 16, 4 x 16 rows in blocks of 7
    sess.reset()
    split = sess.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], chunk=16, head_rows=7)
    logits7 = blockwise_logits(model, sess, c["ids"], c["attention_mask"], 16, 7, 64)
    check_against_own_logits("real/b4 chunk=16 head_rows=7", split, logits7, c["labels"])
    # ... and the two calls agree at the bar the project holds two kernel routes of one model to, on every entry whose query
    # position holds a token (an entry scored from a pad averages every key of its pass: test_score_cpu.py)
    real_query = c["attention_mask"][:, :-1].bool()
    for b in range(B):
        e = O.rel_l2(split.logprobs[b].cpu()[real_query[b]].numpy(), res.logprobs[b].cpu()[real_query[b]].numpy())
        print(f"[score chunked vs one pass] real/b4 row {b}: rel-L2 {e:.3e}")
        assert e <= TOL


def score_case(name, model, capacity, **kw):
    c, loss_ref = case(name)
    B, S = c["ids"].shape
    sess = DecodeSession(model, B, capacity, use_graph=False)
    res = sess.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"], **kw)
    assert torch.equal(res.valid.cpu(), c["labels"][:, 1:] != -100)
    for b in range(B):
        e = O.rel_l2(res.logprobs[b].cpu().numpy(), c["logprobs"][b].numpy())
        print(f"[score vs reference] {name} row {b}: log-prob rel-L2 {e:.3e}")
        assert e <= TOL
    e = abs(float(res.loss) - loss_ref) / abs(loss_ref)
    print(f"[score vs reference] {name}: loss {float(res.loss):.6f} reference {loss_ref:.6f} rel {e:.3e}")
    assert e <= TOL
    return res


@pytest.mark.parametrize("name", ["real/b4", "real/long"])
def test_score_against_reference_real_width(real_gpu, name):
    score_case(name, real_gpu[0], 320)


def test_score_against_reference_true_vocabulary(v65k_gpu):
    score_case("real/v65k", v65k_gpu[0], 64)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_score_against_reference_tiny(dt):
    model, cfg = build_tiny(dt, DEV)
    score_case(f"tiny/{dt}", model, 32)


def test_footprint_full_logits_are_never_resident(v65k_gpu):
    """4 x 512 ids at vocabulary 65024, head_rows = 256: the peak of score() may exceed the peak of prefill() of the same ids on
    the same warmed session by less than HALF of one (B, S, V) fp16 logits tensor (133 MB of 266 MB; a 256-row block is 33 MB)."""
    model, cfg = v65k_gpu
    B, S, V = 4, 512, cfg.vocab_size
    g = torch.Generator().manual_seed(77)
    ids = torch.randint(0, V, (B, S), generator=g)
    sess = DecodeSession(model, B, S, use_graph=False)
    sess.prefill(ids)                                            # warm-up: derived layouts, allocator pools
    sess.reset().score(ids, head_rows=256)
    torch.cuda.synchronize()
    sess.reset()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    sess.prefill(ids)
    torch.cuda.synchronize()
    peak_prefill = torch.cuda.max_memory_allocated() - base
    sess.reset()
    torch.cuda.reset_peak_memory_stats()
    res = sess.score(ids, head_rows=256)
    torch.cuda.synchronize()
    peak_score = torch.cuda.max_memory_allocated() - base
    full = B * S * V * 2
    print(f"[score footprint] prefill peak {peak_prefill / 2**20:.1f} MiB, score peak {peak_score / 2**20:.1f} MiB, "
          f"full fp16 logits {full / 2**20:.1f} MiB")
    assert bool(torch.isfinite(res.loss))
    assert peak_score - peak_prefill < full / 2


@pytest.mark.parametrize("name", ["real/long", "real/b4"])
def test_score_leaves_the_session_as_prefill_does(real_gpu, name):
    """score(ids) then two graph-replayed greedy steps = prefill(ids) then the same steps, tokens and logits bit for bit."""
    model, cfg = real_gpu
    c, _ = case(name)
    B = c["ids"].shape[0]
    runs = []
    for how in ("prefill", "score"):
        sess = DecodeSession(model, B, 320, use_graph=True)
        if how == "prefill":
            last = sess.prefill(c["ids"], attention_mask=c["attention_mask"])
        else:
            last = sess.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"]).logits
        sess.tok.copy_(last.argmax(-1, keepdim=True))
        sess.capture(greedy=True)
        assert sess.graph is not None
        steps = []
        for _ in range(2):
            lg = sess.decode_step(greedy=True)
            steps.append((lg.clone(), sess.tok.clone()))
        runs.append((last.clone(), steps))
    assert torch.equal(runs[0][0], runs[1][0])
    for (la, ta), (lb, tb) in zip(runs[0][1], runs[1][1]):
        assert torch.equal(la, lb) and torch.equal(ta, tb)


def test_low_footprint_session_scores_bit_for_bit():
    model, cfg = build_real(DEV)                                  # its own model: the session drops this one's canonical buffers
    c, _ = case("real/b4")
    B = c["ids"].shape[0]
    plain = DecodeSession(model, B, 64, use_graph=False).score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    low = DecodeSession(model, B, 64, use_graph=False, low_footprint=True)
    first = low.score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    again = low.reset().score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])   # now without the canonical buffers
    assert torch.equal(first.logprobs, plain.logprobs) and torch.equal(again.logprobs, plain.logprobs)
    assert torch.equal(again.loss, plain.loss) and torch.equal(again.logits, plain.logits)


def test_int8_model_and_bf16_model_score_against_their_own_logits():
    # int8 per-channel weights (fp16 activations)
    cfg8 = M.ChatGLM2Config(**G.TINY_INT8_CONFIG)
    m8 = M.create_quant_int8_model(cfg8, dtype=torch.float16)
    G.fill_seeded_int8_(m8.state_dict())
    m8 = m8.to(DEV).eval()
    g = torch.Generator().manual_seed(31)
    B, S = 3, 20
    ids = torch.randint(0, cfg8.vocab_size, (B, S), generator=g)
    attn = torch.ones(B, S, dtype=torch.long)
    attn[1, :6] = 0
    labels = ids.masked_fill(~attn.bool(), -100)
    res = DecodeSession(m8, B, 32, use_graph=False).score(ids, attention_mask=attn, labels=labels)
    check_against_own_logits("int8 tiny", res, own_logits(m8, ids, attn, 32), labels)
    # bf16 activations, int4g32 weights at real width
    mb, cfgb = build_real(DEV, dtype=torch.bfloat16)
    c, _ = case("real/b4")
    resb = DecodeSession(mb, 4, 64, use_graph=False).score(c["ids"], attention_mask=c["attention_mask"], labels=c["labels"])
    check_against_own_logits("bf16 real/b4", resb, own_logits(mb, c["ids"], c["attention_mask"], 64), c["labels"])

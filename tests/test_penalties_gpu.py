"""Sampling controls on the GPU: ``qlinear_logit_penalties`` (csrc/logit_penalties.hip) through ``fused_ops`` / ctypes against the
numpy oracle (tests/_penalty_oracle.py) bit for bit, and the captured "+pen" steps of ``DecodeSession`` /
``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` against a loop written in the tests (eager "logits"-mode step, the oracle on
the host, argmax), against themselves (graph / eager, batch of one, row permutations, mode switches, low footprint) and against the
launch counter.  Every operation of the rules is a single correctly rounded fp32 operation (the division included: the build keeps
hipcc's correctly rounded fp32 division), so exact equality is asked everywhere."""
import numpy as np
import pytest
import torch

import _penalty_oracle as PO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny
from test_model_real_cpu import build_real
from test_penalties_cpu import loop_tokens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NINF = float("-inf")
SPECIAL = [0.0, -0.0, float("inf"), NINF, float("nan"), 1e-30, -1e-30, 65504.0, -65504.0, 3.0e38, 1.0, -1.0]


def make_case(dt, N, B, seed, history="both", ld_extra=0):
    """Logits (B, N) inside a (B, N + ld_extra) buffer, prompt flags, counts up to a few hundred, special values placed on entries
    every rule reaches, and the tokens fed into the step."""
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(B, N + ld_extra, generator=g) * 5).to(PO.DTYPES[dt])
    P = np.zeros((B, N), dtype=bool)
    G = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        n_p, n_g = min(N, 40), min(N, 300)
        if history in ("prompt", "both"):
            P[b, torch.randperm(N, generator=g)[:n_p].numpy()] = True
        if history in ("generated", "both"):
            idx = torch.randperm(N, generator=g)[:n_g].numpy()
            G[b, idx] = torch.randint(1, 400, (len(idx),), generator=g).numpy()
            if history == "both":                                # some ids both in the prompt and generated
                P[b, idx[: max(1, n_g // 10)]] = True
        touched = np.flatnonzero(P[b] | (G[b] > 0))
        spots = list(touched[: len(SPECIAL)]) + list(torch.randperm(N, generator=g)[:len(SPECIAL)].numpy())
        for i, v in zip(spots, SPECIAL + SPECIAL):
            buf[b, int(i)] = v
    tok = torch.randint(0, N, (B,), generator=g)
    return buf, P, G, tok


def load_state(st, P, G):
    words = torch.from_numpy(np.where(P, -(2 ** 31), 0) + G).to(torch.int32)
    st.counts.zero_()
    st.counts[:, :P.shape[1]] = words.to(DEV)


def check_case(dt, N, B, seed, settings, biases, history="both", ld_extra=0, tok_on_bias=True, finished=()):
    buf, P, G, tok = make_case(dt, N, B, seed, history, ld_extra)
    if tok_on_bias:                                              # the increment lands on an entry that is also biased
        for b in range(B):
            if biases[b]:
                tok[b] = sorted(biases[b])[0]
    st = fused_ops.PenaltyState(B, N, DEV).arm([[] for _ in range(B)], settings, biases)
    load_state(st, P, G)
    row_state = None
    if finished:
        row_state = torch.zeros((B, 2), dtype=torch.int32)
        row_state[list(finished), 1] = fused_ops.BatchRows.FINISHED
        row_state = row_state.to(DEV)
    want = PO.to_native(buf)
    dbuf = buf.to(DEV)
    before = _lib.launch_count()
    fused_ops.logit_penalties(dbuf[:, :N], st, tok.to(DEV), row_state)
    assert _lib.launch_count() == before + 1
    got = PO.to_native(dbuf)
    G2 = G.copy()
    for b in range(B):
        if b in finished:
            continue
        G2[b, int(tok[b])] += 1
        want[b, :N] = PO.penalize(want[b, :N], dt, P[b], G2[b], *settings[b], bias=biases[b])
    ok = PO.same(got, want, dt)
    assert ok.all(), (dt, N, B, np.argwhere(~ok)[:8], got[~ok][:8], want[~ok][:8])
    words = st.counts[:, :N].cpu().numpy()
    assert np.array_equal(words & 0x7FFFFFFF, G2) and np.array_equal(words < 0, P)


def mixed_settings(B, N):
    settings = [[(1.3, 0.5, 0.25), (0.7, -0.4, 0.1), (1.0, 0.0, 0.0), (2.5, 0.0, 0.0), (1.0, 1.0, 0.0), (1.0, 0.0, 0.03)][b % 6]
                for b in range(B)]
    biases = []
    for b in range(B):
        k = b % 4
        ids = sorted({(7 * b + 3) % N, (N - 1 - b) % N, (N // 2 + b) % N, b % N})
        biases.append(None if k == 2 else {i: [NINF, -2.5, 4.0, 0.125][(j + b) % 4] for j, i in enumerate(ids[: 1 + k])})
    return settings, biases


# ---- the kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 32])
@pytest.mark.parametrize("N", [7, 1000, 65024, 65025])
@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_kernel_equals_oracle(dt, N, B):
    """All rules together, rows with different settings, prompt + generated history with counts up to 399, -inf / +inf / NaN
    logits, -inf biases, the step's token on a biased entry.  N = 65025 and N = 7 make rows that are not 16-byte aligned."""
    settings, biases = mixed_settings(B, N)
    check_case(dt, N, B, 1000 + N + B, settings, biases)


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("rule", ["repetition", "repetition<1", "presence", "frequency", "bias", "bias-inf", "all"])
@pytest.mark.parametrize("history", ["prompt", "generated", "both"])
def test_every_rule_alone(history, rule, dt):
    B, N = 3, 1000
    s = {"repetition": (1.7, 0.0, 0.0), "repetition<1": (0.6, 0.0, 0.0), "presence": (1.0, 0.9, 0.0), "frequency": (1.0, 0.0, 0.07),
         "bias": (1.0, 0.0, 0.0), "bias-inf": (1.0, 0.0, 0.0), "all": (1.2, -0.3, 0.011)}[rule]
    bias = {"bias": {5: 1.5, 900: -7.0}, "bias-inf": {0: NINF, 999: NINF}, "all": {5: 1.5, 17: NINF}}.get(rule)
    check_case(dt, N, B, 77, [s] * B, [bias] * B, history=history)


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_row_stride_finished_rows_and_null_tok(dt):
    B, N = 4, 1000
    settings, biases = mixed_settings(B, N)
    check_case(dt, N, B, 5, settings, biases, ld_extra=24)                       # ldl > N, rows still 16-byte aligned
    check_case(dt, N, B, 6, settings, biases, ld_extra=3)                        # ldl > N, rows not aligned
    check_case(dt, 65024, B, 7, settings, biases, ld_extra=8, finished=(1, 3))   # finished rows: no count, no write
    # tok = None: nothing is counted
    buf, P, G, _ = make_case(dt, N, B, 8)
    st = fused_ops.PenaltyState(B, N, DEV).arm([[] for _ in range(B)], settings, biases)
    load_state(st, P, G)
    want = PO.to_native(buf)
    d = buf.to(DEV)
    fused_ops.logit_penalties(d, st)
    for b in range(B):
        want[b] = PO.penalize(want[b], dt, P[b], G[b], *settings[b], bias=biases[b])
    assert PO.same(PO.to_native(d), want, dt).all()
    assert np.array_equal(st.generated().cpu().numpy(), G)
    # the full bias list
    full = {i * 13 % N: (NINF if i % 5 == 0 else 0.25 * i - 3) for i in range(fused_ops.LOGIT_BIAS_MAX)}
    assert len(full) == fused_ops.LOGIT_BIAS_MAX
    check_case(dt, N, 2, 9, [(1.1, 0.1, 0.1)] * 2, [full, full])


def test_argument_errors_return_status_codes():
    lib = _lib.get_lib()
    B, N = 2, 100
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    st = fused_ops.PenaltyState(B, N, DEV).arm([[1], [2]], [(1.5, 0.1, 0.1)] * B, [{3: 1.0}, None])
    f16 = _lib.dtype_code(torch.float16)
    cap = fused_ops.LOGIT_BIAS_MAX

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, settings=st.settings.data_ptr(), ids=st.bias_ids.data_ptr(), cap=cap,
             state=st.counts.data_ptr(), lds=st.ld, dtype=f16):
        return lib.qlinear_logit_penalties(logits, b, n, ldl, settings, ids, st.bias_vals.data_ptr(), st.bias_len.data_ptr(), cap,
                                           state, lds, None, None, dtype, _lib.stream_ptr(lg.device))
    before = _lib.launch_count()
    assert call(logits=0) == -1                                 # QL_ERR_NULL_POINTER
    assert call(settings=0) == -1
    assert call(state=0) == -1
    assert call(ids=0) == -1                                    # a bias list is announced (cap > 0) but missing
    assert call(ldl=N - 1) == -2                                # QL_ERR_BAD_SHAPE
    assert call(n=0) == -2
    assert call(lds=N - 1) == -2
    assert call(cap=cap + 1) == -2
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert _lib.launch_count() == before
    torch.cuda.synchronize()
    assert not lg.any() and int(st.generated().sum()) == 0      # nothing ran
    assert call(ids=0, cap=0) == 0 and _lib.launch_count() == before + 1        # no bias lists at all: fine
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        fused_ops.logit_penalties(lg[:1], st)
    with pytest.raises(ValueError):
        fused_ops.logit_penalties(lg, st, torch.zeros(B, dtype=torch.int32, device=DEV))


# ---- the session and the API --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


@pytest.fixture(scope="module")
def real16():
    return build_real(DEV)


PROMPTS = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0], [250]]
PEN = dict(repetition_penalty=[1.5, 1.0, 1.2, 0.8], presence_penalty=[0.0, 0.7, 0.0, -0.2], frequency_penalty=[0.4, 0.0, 0.1, 0.05])


@pytest.mark.parametrize("name", ["tiny", "real"])
def test_greedy_generation_equals_the_loop(name, tiny16, real16):
    """Penalised greedy generate_ids and generate_batch_ids (per-row settings) against eager "logits"-mode steps + the oracle on the
    host + argmax: the adjusted logits are bit-equal, so ties cannot differ."""
    model, cfg = tiny16 if name == "tiny" else real16
    T = 20
    dec = ChatGLMDecoder(cfg, model)
    p = [17, 3, 99, 250, 8, 61]
    base = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    bias = {base[0]: NINF, base[1]: -0.5}
    got = list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, repetition_penalty=1.4, frequency_penalty=0.3,
                                logit_bias=bias))
    assert dec.last_stats["penalties"] is True and "greedy+pen" in dec._session._graphs
    assert got == loop_tokens(model, [p], T, [(1.4, 0.0, 0.3)], [bias])[0]
    assert base[0] not in got and got != base
    # the device loop (no per-token read-back) gives the same tokens
    assert got == list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, sync_every_token=False,
                                        repetition_penalty=1.4, frequency_penalty=0.3, logit_bias=bias))
    bbase = dec.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    bbias = [None, {bbase[1][0]: -1.0}, {bbase[2][0]: NINF}, {bbase[3][1]: NINF, 7: 0.5}]
    bgot = dec.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True, logit_bias=bbias, **PEN)
    assert dec.last_stats["penalties"] is True and "rows+pen" in dec._batch_sessions[4][1]._graphs
    want = loop_tokens(model, PROMPTS, T, list(zip(*(PEN[k] for k in ("repetition_penalty", "presence_penalty", "frequency_penalty")))),
                       bbias)
    assert bgot == want
    assert bbase[2][0] not in bgot[2] and bbase[3][1] not in bgot[3] and bgot != bbase
    # left pads are no prompt tokens: row 1 ([44, 3]) sits behind six pads of id 0
    pen = dec._batch_sessions[4][1].pen
    flagged = [set(torch.nonzero(pen.counts[b, :cfg.vocab_size] < 0).view(-1).tolist()) for b in range(4)]
    assert flagged == [set(q) for q in PROMPTS]


def test_graph_equals_eager(tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=12, ignore_eos=True, logit_bias=[{9: NINF}, None, {1: 2.0}, None], **PEN)
    assert dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=True, **kw) == dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=False, **kw)
    skw = dict(kw, top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])
    g_s = dec.generate_batch_ids(PROMPTS, use_graph=True, **skw)
    assert g_s == dec.generate_batch_ids(PROMPTS, use_graph=False, **skw)
    assert g_s != dec.generate_batch_ids(PROMPTS, use_graph=True, **{k: v for k, v in skw.items() if k not in PEN and k != "logit_bias"})
    p = [17, 3, 99, 250]
    one = dict(max_generated_tokens=12, ignore_eos=True, repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.2, logit_bias={4: -1.0})
    for mode in (dict(greedy=True), dict(seed=77)):
        assert list(dec.generate_ids(p, use_graph=True, **mode, **one)) == list(dec.generate_ids(p, use_graph=False, **mode, **one))


def test_batch_of_one_equals_generate_ids(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250, 8, 61]
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=14, ignore_eos=True, repetition_penalty=1.3, presence_penalty=0.4, frequency_penalty=0.2,
              logit_bias={3: NINF, 99: 1.0})
    assert dec.generate_batch_ids([p], seed=31, **kw) == [list(dec.generate_ids(p, seed=31, **kw))]
    assert dec.generate_batch_ids([p], greedy=True, **kw) == [list(dec.generate_ids(p, greedy=True, **kw))]
    assert "sample+pen" in dec._session._graphs and "greedy+pen" in dec._session._graphs


def test_row_permutation(tiny16):
    """A row's tokens depend neither on its batch position nor on its neighbours' penalties."""
    model, cfg = tiny16
    prompts = PROMPTS + [[12, 13, 14]]
    seeds = [101, 202, 303, 404, 505]
    rp, pp, fp = [1.5, 1.0, 1.2, 0.8, 1.0], [0.0, 0.7, 0.0, -0.2, 0.0], [0.4, 0.0, 0.1, 0.05, 0.0]
    bias = [{9: NINF}, None, {1: 2.0, 2: -2.0}, None, None]
    kw = dict(max_generated_tokens=9, ignore_eos=True)
    top_k = [100, 1, 100, 30, 100]
    base = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, seed=seeds, top_k=top_k, repetition_penalty=rp, presence_penalty=pp,
                                                         frequency_penalty=fp, logit_bias=bias, **kw)
    perm = [3, 0, 4, 2, 1]
    pick = lambda v: [v[i] for i in perm]
    got = ChatGLMDecoder(cfg, model).generate_batch_ids(pick(prompts), seed=pick(seeds), top_k=pick(top_k), repetition_penalty=pick(rp),
                                                        presence_penalty=pick(pp), frequency_penalty=pick(fp), logit_bias=pick(bias), **kw)
    assert got == pick(base)
    # row 4 has every control at its default: it generates what it generates in an unpenalised batch
    plain = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, seed=seeds, top_k=top_k, **kw)
    assert base[4] == plain[4] and base[0] != plain[0]


def test_capture_does_not_count_tokens(tiny16):
    model, cfg = tiny16
    B, n = 3, 7
    prompts = [[5, 9, 200], [44, 3, 1], [100, 101, 102]]
    for mode in ("rows", "greedy"):
        sess = DecodeSession(model, B, 64, use_graph=True)
        assert sess.pen is None
        assert sess.arm_penalties(prompts, 1.3, 0.1, 0.1, None) and sess.pen is not None
        sess.arm_rows([(1, 0.8, 1.0)] * B, [1, 2, 3], [2, n + 5, n + 5])            # row 0 stops after two tokens
        logits = sess.penalize_first(sess.prefill(torch.tensor(prompts)), rows=mode == "rows")
        if mode == "rows":
            sess.sample_rows_first(logits)
        else:
            sess.tok.copy_(logits.argmax(-1, keepdim=True))
        kw = dict(greedy=mode == "greedy", rows=mode == "rows", pen=True)
        sess.capture(**kw)
        assert int(sess.pen.generated().sum()) == 0, "the capture's warm-up runs counted tokens"
        for _ in range(n):
            sess.decode_step(**kw)
        torch.cuda.synchronize()
        assert mode + "+pen" in sess._graphs
        # rows mode: row 0 counted the one token it was fed while live
        assert sess.pen.generated().sum(dim=1).tolist() == ([1, n, n] if mode == "rows" else [n] * B)


def test_launch_accounting(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250]
    T = 9
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2)

    def launches(fn):
        before = _lib.launch_count()
        fn()
        torch.cuda.synchronize()
        return _lib.launch_count() - before

    warm = ChatGLMDecoder(cfg, model)                            # build every lazy layout the steps read before anything is counted
    list(warm.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    warm.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    # eager steps: a penalised token costs exactly one launch more (T - 1 steps and the first token)
    for gen in (lambda d, **k: list(d.generate_ids(p, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k)),
                lambda d, **k: d.generate_batch_ids(PROMPTS, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k)):
        for mode in (dict(greedy=True), dict(seed=3)):
            off = launches(lambda: gen(ChatGLMDecoder(cfg, model), **mode))
            on = launches(lambda: gen(ChatGLMDecoder(cfg, model), **mode, **pen))
            assert on == off + T, (on, off, mode)
    # graphs: an unpenalised generation on a session that holds penalised graphs issues what it issues on a fresh session
    fresh = launches(lambda: list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    dec = ChatGLMDecoder(cfg, model)
    list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, **pen))
    assert launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))) == fresh
    assert set(dec._session._graphs) == {"greedy+pen", "greedy"}
    bfresh = launches(lambda: ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    bdec = ChatGLMDecoder(cfg, model)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, **pen)
    assert launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True)) == bfresh
    # ... and replays the plain graph it captured then: no launch through the library besides prefill and the first token
    again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    pen_again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, **pen))
    assert pen_again == again + 1                                # the first token's penalty launch; the steps are replays


def test_mode_switching_on_one_session(tiny16):
    """Host-sampled, then greedy (penalised and not), then host-sampled again on ONE reused session: every captured step writes a
    logits buffer of its own, and the host-sampled run must read the one its graph writes, not the greedy graph's."""
    model, cfg = tiny16
    p = [17, 3, 99, 250]
    kw = dict(max_generated_tokens=10, ignore_eos=True)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2, logit_bias={5: NINF})

    def host_sampled(d, **extra):
        torch.manual_seed(21)
        return list(d.generate_ids(p, device_sampler=False, **kw, **extra))
    dec = ChatGLMDecoder(cfg, model)
    first, first_pen = host_sampled(dec), host_sampled(dec, **pen)
    sess = dec._session
    greedy_pen = list(dec.generate_ids(p, greedy=True, **kw, **pen))
    greedy = list(dec.generate_ids(p, greedy=True, **kw))
    assert dec._session is sess and {"logits", "greedy", "greedy+pen"} <= set(sess._graphs)
    assert host_sampled(dec) == first
    assert host_sampled(dec, **pen) == first_pen and 5 not in first_pen
    assert list(dec.generate_ids(p, greedy=True, **kw, **pen)) == greedy_pen
    assert list(dec.generate_ids(p, greedy=True, **kw)) == greedy
    assert greedy == list(ChatGLMDecoder(cfg, model).generate_ids(p, greedy=True, **kw))
    assert first == host_sampled(ChatGLMDecoder(cfg, model))


def test_low_footprint_gives_the_same_tokens(tiny16):
    model, cfg = tiny16
    kw = dict(max_generated_tokens=8, ignore_eos=True, seed=[4, 5, 6, 7], logit_bias=[{9: NINF}, None, {1: 2.0}, None], **PEN)
    want = ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, **kw)
    lf_model, _ = build_tiny("f16", DEV)
    got = ChatGLMDecoder(cfg, lf_model, low_footprint=True).generate_batch_ids(PROMPTS, **kw)
    assert got == want
    one = dict(max_generated_tokens=8, ignore_eos=True, greedy=True, repetition_penalty=1.4, logit_bias={3: -1.0})
    assert list(ChatGLMDecoder(cfg, lf_model, low_footprint=True).generate_ids([17, 3, 99], **one)) == \
        list(ChatGLMDecoder(cfg, model).generate_ids([17, 3, 99], **one))

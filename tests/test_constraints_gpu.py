"""History constraints on the GPU: ``qlinear_history_constraints`` (csrc/history_constraints.hip) through ``fused_ops`` / ctypes against
the oracle (tests/_constraints_oracle.py) - logits as integer bit patterns, the history, its length, ``row_state`` and ``live`` all
equal - and the captured "+con" steps of ``DecodeSession`` / ``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` against a loop
written here (eager "logits"-mode step, the oracle on the host, argmax), against themselves (graph / eager, batch of one, row
permutations, mode switches, low footprint) and against the launch counter."""
import random

import numpy as np
import pytest
import torch

import _constraints_oracle as CO
import _penalty_oracle as PO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAN, STOP, MIN = CO.BAN, CO.STOP, CO.MIN
HIST_LD = 8128
FIN = fused_ops.BatchRows.FINISHED


def bits_of(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().view(np.uint16 if t.element_size() == 2 else np.uint32).copy()


def history(rng, L, N, alphabet=5):
    """Ids over a 5-id alphabet (n-grams repeat all the time) with some ids of the whole vocabulary."""
    return [rng.randrange(min(alphabet, N)) if rng.random() < 0.93 else rng.randrange(N) for _ in range(L)]


def sequence_for(rng, h, m, N, match):
    """A sequence of m ids: one the history (after the append) ends with the head of / all of when ``match`` says so and it is long enough."""
    if match == "head" and len(h) >= m - 1:
        return (h[len(h) - (m - 1):] if m > 1 else []) + [rng.randrange(N)]
    if match == "all" and len(h) >= m:
        return h[len(h) - m:]
    return [rng.randrange(min(5, N)) for _ in range(m)]


def make_rows(rng, N, Ls, ns, tok, tables="mixed", prompt="random"):
    """One row per entry of ``Ls`` (the history length before the launch); the table is built against the history as it will be
    after ``tok`` (a list or None) is appended, so that sequences match often."""
    rows = []
    for b, L in enumerate(Ls):
        h = history(rng, L, N)
        after = h + ([tok[b]] if tok is not None and L < HIST_LD else [])
        P = {"random": rng.randrange(0, L + 1), "none": 0, "all": L}[prompt]
        table, min_new = [], 0
        if tables in ("mixed", "ban", "full"):
            count = {"mixed": rng.randrange(0, 5), "ban": 4, "full": 20}[tables]
            for _ in range(count):
                m = 16 if tables == "full" else rng.choice([1, 2, 3, 7, 16])
                table.append((BAN, sequence_for(rng, after, m, N, rng.choice(["head", "head", "none"]))))
        if tables in ("mixed", "stop", "full"):
            count = {"mixed": rng.randrange(0, 3), "stop": 3, "full": 11}[tables]
            for _ in range(count):
                m = 16 if tables == "full" else rng.choice([1, 2, 5, 16])
                table.append((STOP, sequence_for(rng, after, m, N, "all" if rng.random() < (0.08 if tables == "full" else 0.4) else "none")))
        if tables in ("mixed", "min", "full"):
            min_new = rng.choice([len(after) - P, len(after) - P + 1, 0, 3]) if tables != "full" else len(after) - P + 1
            if min_new > 0:
                table.append((MIN, [rng.randrange(N)]))
        assert len(table) <= 32
        rows.append(dict(hist=h, P=P, n=ns[b % len(ns)], min_new=min_new, table=table, N=N))
    return rows


def arm_state(rows):
    st = fused_ops.ConstraintState(len(rows), HIST_LD, DEV)
    st.arm([r["hist"] for r in rows], [(r["n"], r["min_new"], r["table"]) for r in rows])
    st.prompt_len.copy_(torch.tensor([r["P"] for r in rows], dtype=torch.int32))
    return st


def check_launch(dt, N, rows, tok, with_rows=False, finished=(), ld_extra=0, seed=0):
    """One launch on ``rows`` against the oracle: logits bits (sentinel columns past N included), hist, hist_len, row_state, live."""
    B = len(rows)
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(B, N + ld_extra, generator=g) * 4).to(PO.DTYPES[dt])
    st = arm_state(rows)
    row_state = live = rs_t = live_t = None
    if with_rows:
        row_state = [[len(r["hist"]) - r["P"], FIN if b in finished else 0] for b, r in enumerate(rows)]
        live = B - len(finished)
        rs_t, live_t = torch.tensor(row_state, dtype=torch.int32, device=DEV), torch.tensor([live], dtype=torch.int32, device=DEV)
    want = bits_of(buf)
    hist_before = st.hist.cpu()
    dbuf = buf.to(DEV)
    before = _lib.launch_count()
    fused_ops.history_constraints(dbuf[:, :N] if ld_extra else dbuf, st, None if tok is None else torch.tensor(tok, dtype=torch.int64, device=DEV),
                                  rs_t, live_t)
    assert _lib.launch_count() == before + 1
    torch.cuda.synchronize()
    live = CO.launch(want, dt, rows, HIST_LD, tok, row_state, live)
    got = bits_of(dbuf)
    assert np.array_equal(got, want), (dt, N, B, np.argwhere(got != want)[:8])
    assert st.hist_len.tolist() == [len(r["hist"]) for r in rows]
    hist_after = st.hist.cpu()
    for b, r in enumerate(rows):
        L = len(r["hist"])
        assert hist_after[b, :L].tolist() == r["hist"], b
        assert torch.equal(hist_after[b, L:], hist_before[b, L:]), b             # nothing behind the history is written
    if with_rows:
        assert rs_t.tolist() == row_state and int(live_t) == live
    return got, st


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
ALL_L = [0, 1, 255, 256, 257, 1023, 1025, 8127]
GRID = [  # dt, N, B, n per row, L per row (n - 2, n - 1, n next to the fixed lengths)
    ("f16", 65024, 3, [3], [8127, 1023, 255]),
    ("f16", 65024, 33, [0, 1, 2, 3, 16], ALL_L + [1, 2, 3, 14, 15, 16]),
    ("bf16", 65025, 1, [2], [1025]),
    ("bf16", 65025, 3, [16], [14, 15, 16]),
    ("f32", 1000, 33, [3, 2, 16, 1], ALL_L + [0, 1, 2, 3, 14, 15, 16]),
    ("f32", 65024, 3, [1], [8127, 256, 0]),
    ("f16", 7, 3, [1, 2, 3], [0, 1, 257]),
    ("bf16", 7, 33, [2, 3, 16], ALL_L),
    ("f32", 1, 3, [1, 2, 0], [0, 1, 256]),
    ("f16", 1, 1, [1], [8127]),
    ("bf16", 1000, 1, [3], [8127]),
    ("f32", 65025, 3, [2, 3, 0], [1, 2, 1023]),
]


@pytest.mark.parametrize("dt,N,B,ns,Ls", GRID, ids=[f"{c[0]}-N{c[1]}-B{c[2]}" for c in GRID])
def test_kernel_equals_oracle(dt, N, B, ns, Ls):
    rng = random.Random(N * 100 + B)
    Ls = [Ls[b % len(Ls)] for b in range(B)]
    tok = [rng.randrange(min(5, N)) for _ in range(B)]
    check_launch(dt, N, make_rows(rng, N, Ls, ns, tok), tok, seed=B)                                     # generate_ids' launch
    check_launch(dt, N, make_rows(rng, N, Ls, ns, None), None, seed=B + 1)                               # the first token: null tok
    check_launch(dt, N, make_rows(rng, N, Ls, ns, tok), tok, with_rows=True, finished=(B // 2,), seed=B + 2)   # a rows step


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
@pytest.mark.parametrize("rule", ["ngram", "ban", "min", "stop", "full"])
def test_every_rule_alone_and_all_together(rule, dt):
    rng = random.Random(len(rule))
    B, N = 3, 1000
    Ls = [300, 17, 1024]
    tok = [rng.randrange(5) for _ in range(B)]
    ns = {"ngram": [3, 2, 1], "full": [2, 3, 16]}.get(rule, [0])
    rows = make_rows(rng, N, Ls, ns, tok, tables={"ngram": "none"}.get(rule, rule))
    if rule == "full":
        assert all(len(r["table"]) == 32 and all(len(q) == 16 for k, q in r["table"] if k != MIN) for r in rows)
    got, _ = check_launch(dt, N, rows, tok, with_rows=rule in ("stop", "full"), seed=3)
    if rule != "stop":
        assert (got == CO.NEG_INF[dt]).any()                     # the case is not vacuous: something was banned


def test_row_stride_sentinels_finished_rows_and_full_history():
    rng = random.Random(5)
    N, B = 1000, 4
    tok = [1, 2, 3, 4]
    for extra in (24, 3):                                        # ldl > N: the columns behind a row keep their bits
        check_launch("f16", N, make_rows(rng, N, [40, 300, 0, 5], [2], tok), tok, ld_extra=extra, seed=extra)
    # finished rows: bit-untouched - no append, no ban, no stop
    rows = make_rows(rng, N, [40, 300, 70, 5], [1], tok, tables="stop")
    check_launch("bf16", N, rows, tok, with_rows=True, finished=(0, 2), seed=9)
    # L == hist_ld: nothing is appended and the launch goes on with the history as it is
    rows = make_rows(rng, N, [HIST_LD, HIST_LD - 1], [3], tok[:2])
    _, st = check_launch("f32", N, rows, tok[:2], seed=10)
    assert st.hist_len.tolist() == [HIST_LD, HIST_LD]


def test_ids_outside_the_vocabulary_are_stored_and_ban_nothing():
    """tok and history ids of -1 and N: defined behaviour - stored as they are, they never index the logits (every logits index of
    the kernel is range-checked in the thread that stores: csrc/history_constraints.hip, ban())."""
    N = 1000
    h = [-1, N, 3, -1, N, 3, -1]
    rows = [dict(hist=list(h), P=2, n=2, min_new=0, table=[(BAN, [-1, 7])], N=N),          # 2-gram rule names N: outside
            dict(hist=list(h), P=2, n=3, min_new=0, table=[(BAN, [3, N])], N=N),
            dict(hist=list(h), P=2, n=1, min_new=0, table=[], N=N)]
    st = arm_state(rows)
    x = torch.zeros(3, N, dtype=torch.float16, device=DEV)
    want = np.zeros((3, N), dtype=np.uint16)
    fused_ops.history_constraints(x, st, torch.tensor([N, 3, -1], dtype=torch.int64, device=DEV))
    CO.launch(want, "f16", rows, HIST_LD, [N, 3, -1])
    assert np.array_equal(bits_of(x), want)
    assert st.hist[:, :8].tolist() == [h + [N], h + [3], h + [-1]]
    assert np.flatnonzero(want[0]).tolist() == [3] and np.flatnonzero(want[1]).tolist() == [] and np.flatnonzero(want[2]).tolist() == [3]


def test_argument_errors_return_status_codes():
    lib = _lib.get_lib()
    B, N = 2, 100
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    st = fused_ops.ConstraintState(B, 16, DEV).arm([[1, 1], [2]], fused_ops.ConstraintState.check(B, no_repeat_ngram_size=1))
    rs, live = torch.zeros((B, 2), dtype=torch.int32, device=DEV), torch.full((1,), B, dtype=torch.int32, device=DEV)
    f16 = _lib.dtype_code(torch.float16)

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, hist=st.hist.data_ptr(), hist_ld=16, hist_len=st.hist_len.data_ptr(),
             prompt_len=st.prompt_len.data_ptr(), cfg=st.cfg.data_ptr(), seq_tok=st.seq_tok.data_ptr(), seq_len=st.seq_len.data_ptr(),
             seq_kind=st.seq_kind.data_ptr(), seq_count=st.seq_count.data_ptr(), row_state=None, live=None, dtype=f16):
        return lib.qlinear_history_constraints(logits, b, n, ldl, hist, hist_ld, hist_len, prompt_len, cfg, seq_tok, seq_len, seq_kind,
                                               seq_count, None, row_state, live, dtype, _lib.stream_ptr(lg.device))
    before = _lib.launch_count()
    for missing in ("logits", "hist", "hist_len", "prompt_len", "cfg", "seq_tok", "seq_len", "seq_kind", "seq_count"):
        assert call(**{missing: 0}) == -1                        # QL_ERR_NULL_POINTER
    assert call(row_state=rs.data_ptr()) == -1 and call(live=live.data_ptr()) == -1      # one without the other
    assert call(ldl=N - 1) == -2                                # QL_ERR_BAD_SHAPE
    assert call(n=0) == -2
    assert call(hist_ld=0) == -2
    assert call(b=65536) == -2
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert _lib.launch_count() == before
    torch.cuda.synchronize()
    assert not lg.any() and st.hist_len.tolist() == [2, 1]      # nothing ran
    assert call(row_state=rs.data_ptr(), live=live.data_ptr()) == 0 and _lib.launch_count() == before + 1
    torch.cuda.synchronize()
    assert torch.isinf(lg[0]).nonzero().view(-1).tolist() == [1] and torch.isinf(lg[1]).nonzero().view(-1).tolist() == [2]
    with pytest.raises(ValueError):
        fused_ops.history_constraints(lg[:1], st)
    with pytest.raises(ValueError):
        fused_ops.history_constraints(lg, st, row_state=rs)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_stop_sequence_in_a_rows_step(graph):
    """Three greedy rows driven by made-up logits; row 1 has generated its stop sequence after step 3: the launch of step 4 finishes it
    (live 3 -> 2), its tokens end with the sequence, the other rows' tokens are those of a run without the stop."""
    B, N, T = 3, 50, 8
    picks = [[10 + t for t in range(T)], [20, 21, 22, 23, 24, 25, 26, 27], [5, 6, 5, 6, 5, 6, 5, 6]]
    steps = torch.zeros(T, B, N, dtype=torch.float16)
    for t in range(T):
        for b in range(B):
            steps[t, b, picks[b][t]] = 5.0
    steps = steps.to(DEV)
    prompts = [[1, 2, 3], [22, 23], [4]]                         # row 1's prompt ends with the stop sequence: no match in the prompt

    def run(stops):
        rows = fused_ops.BatchRows(B, 16, DEV).arm([(1, 0.8, 1.0)] * B, [1, 2, 3], [T] * B)
        st = fused_ops.ConstraintState(B, 32, DEV).arm(prompts, fused_ops.ConstraintState.check(B, stop_sequences=stops))
        tok = torch.zeros(B, dtype=torch.int64, device=DEV)
        lg = steps[0].clone()
        fused_ops.history_constraints(lg, st, None, rows.row_state, rows.live)
        fused_ops.batch_sample_advance(lg, tok, rows)
        lives = [int(rows.live)]
        body = lambda: (fused_ops.history_constraints(lg, st, tok, rows.row_state, rows.live), fused_ops.batch_sample_advance(lg, tok, rows))
        g = None
        if graph:
            saved = [t.clone() for t in (tok, st.hist_len) + rows.tensors()]
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                body()
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                body()
            for dst, src in zip((tok, st.hist_len) + rows.tensors(), saved):
                dst.copy_(src)
        for t in range(1, T):
            lg.copy_(steps[t])
            g.replay() if graph else body()
            lives.append(int(rows.live))
        counts = rows.row_state[:, 0].tolist()
        return lives, counts, [rows.out_tokens[b, :counts[b]].tolist() for b in range(B)], rows.row_state[:, 1].tolist(), st
    lives, counts, toks, flags, st = run([None, [[9, 9], [22, 23]], None])
    assert lives == [3, 3, 3, 3, 2, 2, 2, 0]                     # the step after the sequence completes; the budget ends the others
    assert counts == [T, 4, T] and toks[1] == [20, 21, 22, 23] and flags[1] & FIN
    assert st.hist_len.tolist() == [3 + T - 1, 2 + 4, 1 + T - 1] and st.hist[1, :6].tolist() == [22, 23, 20, 21, 22, 23]
    _, counts0, toks0, _, _ = run([None, None, [[7, 7]]])
    assert counts0 == [T] * B and toks0 == picks and toks[0] == toks0[0] and toks[2] == toks0[2]


# ---- the session and the API ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


PROMPTS = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0], [250]]
P1, T = [17, 3, 99, 250, 8, 61], 20


def loop_tokens(model, prompts, T, settings, pad_id=0):
    """The test's own loop: prefill the left-padded batch, read the eager step logits, ban what the oracle names for the row's prompt +
    tokens, take the argmax (lowest index on ties), feed it back; a row that has generated a stop sequence stops.  ``settings``: per
    row (n, min_new, table)."""
    B, S, N = len(prompts), max(len(p) for p in prompts), model.config.vocab_size
    ids = torch.full((B, S), pad_id, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    logits = sess.prefill(ids.to(DEV), attention_mask=attn.to(DEV))
    out, done = [[] for _ in range(B)], [False] * B
    for t in range(T):
        raw = PO.to_native(logits)
        tok = []
        for b, (n, min_new, table) in enumerate(settings):
            h = prompts[b] + out[b]
            if not done[b] and CO.stop_index(h, len(prompts[b]), table) is not None:
                done[b] = True
            if done[b]:
                tok.append(0)
                continue
            x = PO.widen(raw[b], "f16")
            for v in CO.bans(h, len(prompts[b]), n, min_new, table):
                x[v] = -np.inf
            tok.append(int(np.argmax(x)))
            out[b].append(tok[-1])
        if t + 1 < T:
            logits = sess.decode_step(torch.tensor(tok, dtype=torch.long, device=DEV)[:, None], greedy=False)
    return out


CONTROLS = {
    "ngram": lambda base: (dict(no_repeat_ngram_size=2), (2, 0, [])),
    "ngram3": lambda base: (dict(no_repeat_ngram_size=3), (3, 0, [])),
    "ban": lambda base: (dict(bad_words_ids=[[base[2], base[3]], [base[0]]]), (0, 0, [(BAN, [base[2], base[3]]), (BAN, [base[0]])])),
    "stop": lambda base: (dict(stop_sequences=[[base[4], base[5]]]), (0, 0, [(STOP, [base[4], base[5]])])),
    "all": lambda base: (dict(no_repeat_ngram_size=2, bad_words_ids=[[base[1], base[2]]], stop_sequences=[[base[9], 255]]),
                         (2, 0, [(BAN, [base[1], base[2]]), (STOP, [base[9], 255])])),
}


@pytest.mark.parametrize("control", sorted(CONTROLS))
def test_greedy_generation_equals_the_loop(control, tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    kw = dict(max_generated_tokens=T, greedy=True, ignore_eos=True)
    base = list(dec.generate_ids(P1, **kw))
    assert dec.last_stats["constraints"] is False and dec._session.con is None
    args, setting = CONTROLS[control](base)
    got = list(dec.generate_ids(P1, **kw, **args))
    want = loop_tokens(model, [P1], T, [setting])[0]
    assert got == want and got != base and dec.last_stats["constraints"] is True
    if control != "stop":
        assert "greedy+con" in dec._session._graphs
        assert got == list(dec.generate_ids(P1, sync_every_token=False, **kw, **args))       # the device loop: the same tokens
    # per-row settings in one batch: row 0 the control, the others defaults / a 2-gram rule
    prompts = [P1] + PROMPTS[1:]
    bbase = dec.generate_batch_ids(prompts, **kw)
    bargs = {k: [v, None, None, None] if k in ("bad_words_ids", "stop_sequences") else [v, 0, 2, 0] for k, v in args.items()}
    bargs.setdefault("no_repeat_ngram_size", [0, 0, 2, 0])
    bgot = dec.generate_batch_ids(prompts, **kw, **bargs)
    n2 = bargs["no_repeat_ngram_size"][2]
    assert bgot == loop_tokens(model, prompts, T, [setting, (0, 0, []), (n2, 0, []), (0, 0, [])])
    assert bgot[0] != bbase[0] and bgot[1] == bbase[1] and bgot[3] == bbase[3]
    assert "rows+con" in dec._batch_sessions[4][1]._graphs


def test_min_new_tokens_equals_the_loop(tiny16):
    model, cfg = tiny16
    base = list(ChatGLMDecoder(cfg, model).generate_ids(P1, max_generated_tokens=T, greedy=True, ignore_eos=True))
    eos = base[2]
    assert eos not in base[:2]
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos)
    assert list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True)) == base[:3]
    got = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, min_new_tokens=6))
    want = loop_tokens(model, [P1], T, [(0, 6, [(MIN, [eos])])])[0]
    cut = next((i + 1 for i, v in enumerate(want) if v == eos), T)
    assert got == want[:cut] and len(got) >= 6 and eos not in got[:6]
    bwant = loop_tokens(model, [P1, P1], T, [(0, 6, [(MIN, [eos])]), (0, 0, [])])
    bwant = [w[:next((i + 1 for i, v in enumerate(w) if v == eos), T)] for w in bwant]
    bgot = dec.generate_batch_ids([P1, P1], max_generated_tokens=T, greedy=True, min_new_tokens=[6, 0])
    assert bgot == bwant and len(bgot[1]) == 3 and len(bgot[0]) >= 6


def test_graph_equals_eager(tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    base = dec.generate_batch_ids(PROMPTS, max_generated_tokens=12, greedy=True, ignore_eos=True)
    kw = dict(max_generated_tokens=12, ignore_eos=True, no_repeat_ngram_size=[2, 0, 3, 1], bad_words_ids=[None, [[base[1][1], base[1][2]]], None, None],
              stop_sequences=[None, None, [[base[2][0]]], None])             # row 2 stops on its first token
    g = dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=True, **kw)
    assert g == dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=False, **kw) and g != base
    assert dec.last_stats["stop_sequence"] == [None, None, 0, None] and g[2] == base[2][:1]
    skw = dict(kw, top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])
    assert dec.generate_batch_ids(PROMPTS, use_graph=True, **skw) == dec.generate_batch_ids(PROMPTS, use_graph=False, **skw)
    one = dict(max_generated_tokens=12, ignore_eos=True, no_repeat_ngram_size=2, bad_words_ids=[[base[0][0]]], repetition_penalty=1.2)
    for mode in (dict(greedy=True), dict(seed=77)):
        assert list(dec.generate_ids(P1, use_graph=True, **mode, **one)) == list(dec.generate_ids(P1, use_graph=False, **mode, **one))


def test_batch_of_one_equals_generate_ids(tiny16):
    model, cfg = tiny16
    dec = ChatGLMDecoder(cfg, model)
    base = list(dec.generate_ids(P1, max_generated_tokens=14, greedy=True, ignore_eos=True))
    kw = dict(max_generated_tokens=14, ignore_eos=True, no_repeat_ngram_size=2, bad_words_ids=[[base[0]]], stop_sequences=[[base[1], 255]])
    assert dec.generate_batch_ids([P1], seed=31, **kw) == [list(dec.generate_ids(P1, seed=31, **kw))]
    assert dec.generate_batch_ids([P1], greedy=True, **kw) == [list(dec.generate_ids(P1, greedy=True, **kw))]
    assert "sample+con" in dec._session._graphs and "greedy+con" in dec._session._graphs
    # a stop sequence ends both the same way
    g = list(dec.generate_ids(P1, max_generated_tokens=14, greedy=True, ignore_eos=True))
    stop = dict(max_generated_tokens=14, greedy=True, ignore_eos=True, stop_sequences=[[g[3], g[4]]])
    a = list(dec.generate_ids(P1, **stop))
    assert dec.generate_batch_ids([P1], **stop) == [a] and a[-2:] == [g[3], g[4]] and len(a) <= 5


def test_row_permutation(tiny16):
    """A row's tokens depend neither on its batch position nor on its neighbours' constraints."""
    model, cfg = tiny16
    prompts = PROMPTS + [[12, 13, 14]]
    seeds = [101, 202, 303, 404, 505]
    top_k = [100, 1, 100, 30, 100]
    kw = dict(max_generated_tokens=10, ignore_eos=True)
    plain = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, seed=seeds, top_k=top_k, **kw)
    ns, mins = [2, 0, 1, 3, 0], [0, 0, 0, 0, 0]
    bans = [None, [[plain[1][0]], [plain[1][2], plain[1][3]]], None, [[7]], None]
    stops = [None, None, [[plain[2][4]]], None, None]
    base = ChatGLMDecoder(cfg, model).generate_batch_ids(prompts, seed=seeds, top_k=top_k, no_repeat_ngram_size=ns, bad_words_ids=bans,
                                                         stop_sequences=stops, min_new_tokens=mins, **kw)
    perm = [3, 0, 4, 2, 1]
    pick = lambda v: [v[i] for i in perm]
    got = ChatGLMDecoder(cfg, model).generate_batch_ids(pick(prompts), seed=pick(seeds), top_k=pick(top_k), no_repeat_ngram_size=pick(ns),
                                                        bad_words_ids=pick(bans), stop_sequences=pick(stops), min_new_tokens=pick(mins), **kw)
    assert got == pick(base)
    assert base[4] == plain[4] and base[1] != plain[1]           # row 4 has every control at its default


def test_capture_appends_nothing_and_stops_nothing(tiny16):
    model, cfg = tiny16
    B, n = 3, 7
    prompts = [[5, 9, 200], [44, 3, 1], [100, 101, 102]]
    first = DecodeSession(model, B, 64, use_graph=False).prefill(torch.tensor(prompts)).argmax(-1).tolist()
    for mode in ("rows", "greedy"):
        sess = DecodeSession(model, B, 64, use_graph=True)
        assert sess.con is None
        # rows: every row's first token is its stop sequence - the first step, and so every warm-up run of the capture, stops every row;
        # greedy: the 1-gram rule
        assert sess.arm_constraints(prompts, 1 if mode == "greedy" else 0, None, [[[f]] for f in first], 0, None) and sess.con is not None
        sess.arm_rows([(1, 0.8, 1.0)] * B, [1, 2, 3], [n + 5] * B)
        logits = sess.constrain_first(sess.prefill(torch.tensor(prompts)), rows=mode == "rows")
        if mode == "rows":
            sess.sample_rows_first(logits)
        else:
            sess.tok.copy_(logits.argmax(-1, keepdim=True))
        kw = dict(greedy=mode == "greedy", rows=mode == "rows", con=True)
        live, state = int(sess.rows.live), sess.rows.row_state.clone()
        sess.capture(**kw)
        torch.cuda.synchronize()
        assert sess.con.hist_len.tolist() == [3] * B, "the capture's warm-up runs appended tokens"
        assert int(sess.rows.live) == live and torch.equal(sess.rows.row_state, state), "the capture's warm-up runs stopped a row"
        for _ in range(2):
            sess.decode_step(**kw)
        torch.cuda.synchronize()
        assert mode + "+con" in sess._graphs
        if mode == "rows":
            assert sess.rows.out_tokens[:, 0].tolist() == first and int(sess.rows.live) == 0
            assert sess.con.hist_len.tolist() == [4] * B and sess.rows.row_state[:, 0].tolist() == [1] * B
        else:
            assert sess.con.hist_len.tolist() == [5] * B
            h = sess.con.hist[:, :5].tolist()
            assert all(len(set(r)) == 5 for r in h)              # the 1-gram rule: no id twice, prompt included


# launches of the same calls on the commit before this feature (tiny fp16 model, T = 9): generate_ids greedy / sampled and
# generate_batch_ids greedy / sampled with use_graph=False; generate_ids greedy and generate_batch_ids sampled on fresh graph sessions
PARENT_EAGER_LAUNCHES = [125, 126, 172, 172]
PARENT_GRAPH_LAUNCHES = [47, 64]


def test_launch_accounting(tiny16):
    model, cfg = tiny16
    p = [17, 3, 99, 250]
    T = 9
    con = dict(no_repeat_ngram_size=2, bad_words_ids=[[5, 6]])

    def launches(fn):
        before = _lib.launch_count()
        fn()
        torch.cuda.synchronize()
        return _lib.launch_count() - before

    warm = ChatGLMDecoder(cfg, model)                            # build every lazy layout the steps read before anything is counted
    list(warm.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    warm.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    # eager steps: a constrained token costs exactly one launch more (T - 1 steps and the first token)
    gens = (lambda d, **k: list(d.generate_ids(p, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k)),
            lambda d, **k: d.generate_batch_ids(PROMPTS, max_generated_tokens=T, ignore_eos=True, use_graph=False, **k))
    offs = []
    for gen in gens:
        for mode in (dict(greedy=True), dict(seed=3)):
            dec = ChatGLMDecoder(cfg, model)
            off = launches(lambda: gen(dec, **mode))
            assert dec.last_stats["constraints"] is False
            on = launches(lambda: gen(ChatGLMDecoder(cfg, model), **mode, **con))
            assert on == off + T, (on, off, mode)
            offs.append(off)
    # every new argument at its default: exactly the launches of the commit before the constraints (counted there, same calls)
    assert offs == PARENT_EAGER_LAUNCHES, offs
    # graphs: an unconstrained generation on a session that holds constrained graphs issues what it issues on a fresh session
    fresh = launches(lambda: list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    dec = ChatGLMDecoder(cfg, model)
    list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, **con))
    assert launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))) == fresh
    assert set(dec._session._graphs) == {"greedy+con", "greedy"}
    bfresh = launches(lambda: ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    assert [fresh, bfresh] == PARENT_GRAPH_LAUNCHES, (fresh, bfresh)
    bdec = ChatGLMDecoder(cfg, model)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, **con)
    assert launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True)) == bfresh
    again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    con_again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True, **con))
    assert con_again == again + 1                                # the first token's launch; the steps are replays
    # with defaults nothing is armed or allocated
    d = ChatGLMDecoder(cfg, model)
    list(d.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True, no_repeat_ngram_size=0, bad_words_ids=None,
                        stop_sequences=None, min_new_tokens=0))
    d.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True, min_new_tokens=5, bad_words_ids=[None] * 4)
    assert d._session.con is None and d._batch_sessions[4][1].con is None and d.last_stats["constraints"] is False


def test_mode_switching_on_one_session(tiny16):
    """Plain, "+pen", "+con" and "+con+lp" generations on ONE reused session: each mode's graph keeps returning its own tokens."""
    model, cfg = tiny16
    kw = dict(max_generated_tokens=10, ignore_eos=True, greedy=True)
    pen = dict(repetition_penalty=1.3, frequency_penalty=0.2)
    con = dict(no_repeat_ngram_size=2, bad_words_ids=[[197]])
    dec = ChatGLMDecoder(cfg, model)
    runs = [dict(), pen, con, dict(con, logprobs=3), dict(pen, **con)]
    first = [list(dec.generate_ids(P1, **kw, **r)) for r in runs]
    sess = dec._session
    assert {"greedy", "greedy+pen", "greedy+con", "greedy+con+lp", "greedy+pen+con"} <= set(sess._graphs)
    assert first[2] == first[3] and first[0] != first[2] and first[1] != first[4]
    for r, want in list(zip(runs, first))[::-1] + list(zip(runs, first)):
        assert list(dec.generate_ids(P1, **kw, **r)) == want
    assert dec._session is sess
    fresh = ChatGLMDecoder(cfg, model)
    assert [list(fresh.generate_ids(P1, **kw, **r)) for r in (runs[2], runs[0])] == [first[2], first[0]]
    # the host-decides path applies the launch to the logits it gets back
    torch.manual_seed(21)
    a = list(dec.generate_ids(P1, device_sampler=False, max_generated_tokens=10, ignore_eos=True, **con))
    torch.manual_seed(21)
    assert a == list(ChatGLMDecoder(cfg, model).generate_ids(P1, device_sampler=False, max_generated_tokens=10, ignore_eos=True, **con))
    assert 197 not in a and len(set(zip(P1 + a, (P1 + a)[1:]))) == len(P1 + a) - 1


def test_low_footprint_gives_the_same_tokens(tiny16):
    model, cfg = tiny16
    kw = dict(max_generated_tokens=8, ignore_eos=True, seed=[4, 5, 6, 7], no_repeat_ngram_size=[2, 0, 1, 3], bad_words_ids=[[9], [171]])
    want = ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, **kw)
    lf_model, _ = build_tiny("f16", DEV)
    assert ChatGLMDecoder(cfg, lf_model, low_footprint=True).generate_batch_ids(PROMPTS, **kw) == want
    one = dict(max_generated_tokens=8, ignore_eos=True, greedy=True, no_repeat_ngram_size=2, bad_words_ids=[[3, 4]])
    assert list(ChatGLMDecoder(cfg, lf_model, low_footprint=True).generate_ids([17, 3, 99], **one)) == \
        list(ChatGLMDecoder(cfg, model).generate_ids([17, 3, 99], **one))

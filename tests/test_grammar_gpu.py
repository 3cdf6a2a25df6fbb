"""Regex-constrained generation on the GPU: ``qlinear_grammar_mask`` (csrc/grammar_mask.hip) through ``fused_ops`` / ctypes against the
oracle (tests/_grammar_oracle.py) - logits as integer bit patterns, the states and the tickets all equal - the exactly-once advance of
the state over 50 launches, eager and as a replayed graph, and the captured "+gr" steps of ``DecodeSession`` / ``ChatGLMDecoder.generate_ids``
/ ``generate_batch_ids`` against a loop written here (eager "logits"-mode step, the oracle's mask on the host, argmax), against themselves
(graph / eager, batch of one, row permutations, together with the other controls) and against the launch counter."""
import functools
import random
import re

import numpy as np
import pytest
import torch

import _grammar_oracle as GO
import _penalty_oracle as PO
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd import grammar as G
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIN = fused_ops.BatchRows.FINISHED
CHUNK = fused_ops.GRAMMAR_CHUNK
SINGLES = b"yesnoABCD-0123456789abcde,x"
KERNEL_PATTERNS = ["(yes|no)", "[A-D]", "-?[0-9]{1,3}", "[a-d]*", "a.c", "[^a]+,", "(ab|cd)*e?", ".*", '\\{("[a-z]+":("[^"]*"|-?[0-9]+))?\\}']
# n_states * n_classes exactly at GRAMMAR_TABLE_MAX: 2032 states of the run of x, 15 inside the alternatives, the accepting one; 8 classes
LIMIT_PATTERN = "x{2031}(a|bb|ccc|dddd|eeeee|ffffff)"


def bits_of(t: torch.Tensor) -> np.ndarray:
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16 if t.element_size() == 2 else torch.int32).numpy().view(np.uint16 if t.element_size() == 2 else np.uint32).copy()


@functools.lru_cache(maxsize=None)
def dfa_of(pattern):
    return G.compile_regex(pattern)


@functools.lru_cache(maxsize=None)
def vocab_of(n, seed=0):
    return GO.make_vocab(n, seed=seed, singles=SINGLES)


def arm_state(rows, vocab):
    st = fused_ops.GrammarState(len(rows), G.token_byte_table(vocab), DEV).arm([r["dfa"] for r in rows], [r["eos"] for r in rows])
    st.state.copy_(torch.tensor([r["state"] for r in rows], dtype=torch.int32))
    return st


def check_launch(dt, N, rows, vocab, tok, finished=None, ld_extra=0, seed=0):
    """One launch on ``rows`` against the oracle: logits bits (sentinel columns past N included), every state, every ticket."""
    B = len(rows)
    g = torch.Generator().manual_seed(seed)
    buf = (torch.randn(B, N + ld_extra, generator=g) * 4).to(PO.DTYPES[dt])
    st = arm_state(rows, vocab)
    row_state = rs_t = None
    if finished is not None:
        row_state = [[0, FIN if b in finished else 0] for b in range(B)]
        rs_t = torch.tensor(row_state, dtype=torch.int32, device=DEV)
    want = bits_of(buf)
    before_states = [r["state"] for r in rows]
    dbuf = buf.to(DEV)
    before = _lib.launch_count()
    fused_ops.grammar_mask(dbuf[:, :N] if ld_extra else dbuf, st, None if tok is None else torch.tensor(tok, dtype=torch.int64, device=DEV), rs_t)
    assert _lib.launch_count() == before + 1
    torch.cuda.synchronize()
    GO.launch(want, dt, rows, vocab, tok, row_state)
    got = bits_of(dbuf)
    assert np.array_equal(got, want), (dt, N, B, np.argwhere(got != want)[:8])
    assert st.states() == [r["state"] for r in rows], (dt, N, B, before_states)
    assert st.ticket.tolist() == [0] * B
    if rs_t is not None:
        assert rs_t.tolist() == row_state                       # the launch reads the flags, it never writes them
    return st


def random_rows(rng, B, N, vocab, patterns=KERNEL_PATTERNS):
    rows = []
    for _ in range(B):
        dfa = dfa_of(rng.choice(patterns))
        state = rng.choice([0, 0, rng.randrange(dfa.n_states), rng.randrange(dfa.n_states), -1])
        rows.append(dict(dfa=dfa, state=state, eos=rng.choice([-1, rng.randrange(N), N - 1]), N=N))
    return rows


def random_tok(rng, rows, vocab, N):
    """One fed id per row: often one the row's state survives, else any id, an empty one, the end id, -1 or an id outside the table."""
    tok = []
    for r in rows:
        kind = rng.choice(["ok", "ok", "any", "empty", "eos", "neg", "past", "huge"])
        ok = sorted(GO.allowed_ids(r["dfa"], r["state"], vocab, -1, min(N, 300))) if kind == "ok" and r["state"] >= 0 else []
        empties = [i for i in range(min(N, len(vocab))) if not vocab[i]]
        tok.append(rng.choice(ok) if ok else rng.choice(empties) if kind == "empty" and empties else r["eos"] if kind == "eos"
                   else -1 if kind == "neg" else N + rng.randrange(3) if kind == "past" else 2 ** 40 if kind == "huge" else rng.randrange(N))
    return tok


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1023, 1025, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 3])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_kernel_equals_oracle(dt, B, N):
    rng = random.Random(f"{dt}/{B}/{N}")
    vocab = vocab_of(N)
    for trial, ld_extra in enumerate((0, 5)):
        rows = random_rows(rng, B, N, vocab)
        tok = None if trial == 0 and N % 2 else random_tok(rng, rows, vocab, N)
        check_launch(dt, N, rows, vocab, tok, ld_extra=ld_extra if B > 1 else 0, seed=N + trial)


def test_kernel_at_the_real_vocabulary_size():
    N = 65024
    rng = random.Random(65024)
    vocab = vocab_of(N)
    rows = [dict(dfa=dfa_of(KERNEL_PATTERNS[-1]), state=0, eos=N - 1, N=N), dict(dfa=dfa_of("[^a]+,"), state=1, eos=2, N=N)]
    tok = [sorted(GO.allowed_ids(rows[0]["dfa"], 0, vocab, -1, 400))[0], rng.randrange(N)]
    check_launch("f16", N, rows, vocab, tok, ld_extra=3)


def test_a_vocabulary_table_shorter_or_longer_than_the_logits():
    rng = random.Random(9)
    for N, n_vocab in ((600, 520), (600, 700), (CHUNK, CHUNK - 1)):
        vocab = vocab_of(n_vocab, seed=1)
        rows = random_rows(rng, 3, N, vocab)
        check_launch("f16", N, rows, vocab, [n_vocab - 1, n_vocab, N - 1])          # ids past the table: empty - fed: no move, masked


CASES = {
    # name: (rows as (pattern or None, state as bytes walked from the start or an int, eos - "empty": the id of an empty token, as a real
    # end token is), fed ids as token bytes / ints / "eos" = the row's end id / None, finished)
    "tok_null": ([("(yes|no)", b"", 7), ("[A-D]", b"", -1), ("-?[0-9]{1,3}", b"", 0)], None, None),
    "fed_out_of_range": ([("(yes|no)", b"y", 7), ("[A-D]", b"", 3), ("-?[0-9]{1,3}", b"-", 0)], [-1, 10 ** 6, 2 ** 40], None),
    "fed_empty_or_end_id": ([("(yes|no)", b"ye", 7), ("[A-D]", b"A", "empty"), ("-?[0-9]{1,3}", b"-1", "empty")], [b"", "eos", "eos"], None),
    "dead_state": ([("(yes|no)", -1, 7), ("[A-D]", -1, -1), ("-?[0-9]{1,3}", b"1", 0)], [b"y", b"A", b"x"], None),
    "accepting_without_continuation": ([("(yes|no)", b"ye", 7), ("[A-D]", b"", 3), ("-?[0-9]{1,3}", b"12", 0)], [b"s", b"D", b"3"], None),
    "no_end_id": ([("(yes|no)", b"no", -1), ("[a-d]*", b"abc", -1), (".*", b"", -1)], [b"", b"d", b"yes"], None),
    "finished_rows": ([("(yes|no)", b"y", 7), ("[A-D]", b"", 3), ("-?[0-9]{1,3}", b"-", 0)], [b"e", b"B", b"4"], {0, 2}),
    "rows_without_a_grammar": ([(None, 0, 7), ("[A-D]", b"", 3), (None, 5, -1)], [b"e", b"B", b"4"], None),
    "a_pattern_per_row": ([("(ab|cd)*e?", b"ab", 1), ("a.c", b"a", 2), ("[^a]+,", b"b", 3), (KERNEL_PATTERNS[-1], b'{"k":', 4)],
                          [b"cd", "é".encode(), b"c,", b"-1"], None),
}


@pytest.mark.parametrize("dt", ["f16", "f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_kernel_cases(case, dt):
    N = CHUNK + 9                                               # two workgroups per row
    extra = (b"", b"e", b"s", b"D", b"3", b"d", b"yes", b"B", b"4", b"cd", "é".encode(), b"c,", b"-1", b"y", b"A", b"x")
    vocab = GO.make_vocab(N, seed=3, singles=SINGLES + b'{}":k', extra=extra)
    spec, fed, finished = CASES[case]
    rows = []
    for pattern, start, eos in spec:
        dfa = None if pattern is None else dfa_of(pattern)
        state = start if isinstance(start, int) else GO.walk(dfa, 0, start)
        assert pattern is None or isinstance(start, int) or state >= 0, (case, pattern, start)
        rows.append(dict(dfa=dfa, state=state, eos=[i for i, t in enumerate(vocab) if not t][1] if eos == "empty" else eos, N=N))
    tok = None if fed is None else [vocab.index(t) if isinstance(t, bytes) else rows[b]["eos"] if t == "eos" else t for b, t in enumerate(fed)]
    before = [r["state"] for r in rows]
    st = check_launch(dt, N, rows, vocab, tok, finished=finished, ld_extra=2)
    after = st.states()
    if case == "accepting_without_continuation":
        for b, r in enumerate(rows):                            # only the end id survives
            assert GO.allowed_ids(r["dfa"], after[b], vocab, r["eos"], N) == {r["eos"]}
    if case == "dead_state":
        assert after == [-1, -1, -1]
    if case in ("fed_out_of_range", "fed_empty_or_end_id", "tok_null"):
        assert after == before
    if case == "finished_rows":
        assert after[0] == before[0] and after[2] == before[2] and after[1] != before[1]
    if case == "rows_without_a_grammar":
        assert after[0] == 0 and after[2] == 5 and after[1] == GO.walk(rows[1]["dfa"], 0, b"B")


@pytest.mark.parametrize("dt", ["f16", "f32"])
def test_a_table_at_the_limit(dt):
    dfa = dfa_of(LIMIT_PATTERN)
    assert dfa.n_states * dfa.n_classes == fused_ops.GRAMMAR_TABLE_MAX == 16384 and (dfa.n_states, dfa.n_classes) == (2048, 8)
    N = CHUNK + 40
    vocab = GO.make_vocab(N, seed=5, singles=b"xabcdef", alphabet=b"xxxxxxabcdef", extra=(b"x" * 40, b"xa", b"xbb", b"ee", b"fff"))
    deep = [GO.walk(dfa, 0, b"x" * k) for k in (2031, 2030, 1991, 7)]
    last = GO.walk(dfa, 0, b"x" * 2031 + b"fffff")
    assert min(deep) >= 0 and last >= 0
    rows = [dict(dfa=dfa, state=s, eos=e, N=N) for s, e in zip(deep + [last, 0], (3, -1, 4, 5, 6, 7))]
    tok = [vocab.index(b"e"), vocab.index(b"xbb"), vocab.index(b"x" * 40), vocab.index(b"x"), vocab.index(b"f"), -1]
    st = check_launch(dt, N, rows, vocab, tok)
    assert st.states()[2] == GO.walk(dfa, 0, b"x" * 2031) and dfa.accept[st.states()[4]] and st.states()[1] >= 0


def test_argument_errors_and_no_launch():
    lib = _lib.get_lib()
    B, N = 2, 40
    vocab = vocab_of(N)
    st = arm_state([dict(dfa=dfa_of("[A-D]"), state=0, eos=-1, N=N)] * 2, vocab)
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    f16 = _lib.dtype_code(torch.float16)

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, off=st.tok_off.data_ptr(), data=st.tok_bytes.data_ptr(), n_tok=st.n_tok, n_bytes=st.n_bytes,
             class_of=st.class_of.data_ptr(), table=st.table.data_ptr(), accept=st.accept.data_ptr(), cfg=st.cfg.data_ptr(),
             state=st.state.data_ptr(), ticket=st.ticket.data_ptr(), dtype=f16):
        return lib.qlinear_grammar_mask(logits, b, n, ldl, off, data, n_tok, n_bytes, class_of, table, accept, cfg, state, ticket, None, None,
                                        dtype, _lib.stream_ptr(lg.device))
    before = _lib.launch_count()
    for missing in ("logits", "off", "data", "class_of", "table", "accept", "cfg", "state", "ticket"):
        assert call(**{missing: 0}) == -1                        # QL_ERR_NULL_POINTER
    assert call(ldl=N - 1) == -2 and call(n=0) == -2 and call(n_tok=0) == -2 and call(n_bytes=-1) == -2 and call(b=65536) == -2
    assert call(table=st.table.data_ptr() + 2) == -5            # QL_ERR_MISALIGNED
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert _lib.launch_count() == before
    torch.cuda.synchronize()
    assert not lg.any() and st.states() == [0, 0]               # nothing ran
    assert call() == 0 and _lib.launch_count() == before + 1
    torch.cuda.synchronize()
    allowed = sorted(GO.allowed_ids(dfa_of("[A-D]"), 0, vocab, -1, N))
    assert allowed and (~torch.isinf(lg[0])).nonzero().view(-1).tolist() == allowed == (~torch.isinf(lg[1])).nonzero().view(-1).tolist()
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(lg[:1], st)
    with pytest.raises(ValueError):
        fused_ops.grammar_mask(lg.cpu(), st)


# ---- the state advances exactly once per launch --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_exactly_once_advance(graph):
    """Two rows fed 50 tokens of a string of their language one launch at a time, five workgroups per row: after EVERY launch the state
    is the oracle's - a workgroup that saw the new state, a double advance or a lost one shows - and every ticket is back at 0."""
    B, N, T = 2, 4 * CHUNK + 3, 50
    vocab = vocab_of(N, seed=2)
    patterns = ["([a-d]{1,3}[ ,])*[a-d]{0,3}", "(-?[0-9]{1,3},|yes|no| )*"]
    rng = random.Random(50)
    rows = [dict(dfa=dfa_of(p), state=0, eos=-1, N=N) for p in patterns]
    feeds, states = [], [[0, 0]]
    for t in range(T):                                          # a random walk through each language, token by token
        tok = []
        for b, r in enumerate(rows):
            ok = sorted(GO.allowed_ids(r["dfa"], states[-1][b], vocab, -1, N))
            long = [i for i in ok if len(vocab[i]) > 1]
            tok.append(rng.choice(long if long and rng.random() < 0.7 else ok))
        feeds.append(tok)
        states.append([GO.walk(r["dfa"], states[-1][b], vocab[tok[b]]) for b, r in enumerate(rows)])
    assert all(s >= 0 for row in states for s in row) and len({tuple(s) for s in states}) > 3
    st = arm_state(rows, vocab)
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    fused_ops.grammar_mask(lg, st)                              # the first token's launch: nothing moves
    torch.cuda.synchronize()
    assert st.states() == [0, 0]
    body = lambda: fused_ops.grammar_mask(lg, st, tok)
    g = None
    if graph:
        saved = st.state.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            body()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            body()
        st.state.copy_(saved)
    for t in range(T):
        tok.copy_(torch.tensor(feeds[t], dtype=torch.int64))
        lg.zero_()
        g.replay() if graph else body()
        torch.cuda.synchronize()
        assert st.states() == states[t + 1], t
        if t in (0, 17, T - 1):                                 # ... and the mask is the new state's
            for b, r in enumerate(rows):
                assert (~torch.isinf(lg[b])).nonzero().view(-1).tolist() == sorted(GO.allowed_ids(r["dfa"], states[t + 1][b], vocab, -1, N))
    assert st.ticket.tolist() == [0] * B


# ---- the session and the API ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


P1 = [17, 3, 99, 250, 8, 61]
PROMPTS = [[5, 9, 200, 31, 7, 44, 3, 12], [44, 3], [100, 101, 102, 0], [250]]
LANGUAGES = {"(yes|no)": 3, "[A-D]": 1, "-?[0-9]{1,3}": 4}       # a finite language and its longest word, in bytes
WORDS = (b"yes", b"no", b"ye", b"es", b"12", b"-1", b"007", b"AB", b"noo", b"-")


@functools.lru_cache(maxsize=None)
def tiny_vocab(n=256):
    vocab = GO.make_vocab(n, seed=11, singles=b"yesnoABCD-0123456789", extra=WORDS)
    eos = [i for i, t in enumerate(vocab) if not t][1]
    assert eos not in P1 and all(eos not in q for q in PROMPTS + [[12, 13, 14]])     # (so no prompt feeds it to the model)
    return vocab, eos


def decoder(tiny16, **kw):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    return ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=TOKEN_BYTES(), **kw)


@functools.lru_cache(maxsize=None)
def TOKEN_BYTES():
    return G.token_byte_table(tiny_vocab()[0])                  # one table object: a session keeps its GrammarState across decoders' calls


def check_row(pattern, ids, eos, vocab, state):
    assert ids and ids[-1] == eos and eos not in ids[:-1], (pattern, ids)
    text = b"".join(vocab[i] for i in ids[:-1])
    assert re.fullmatch(pattern.encode(), text), (pattern, text)
    assert state == "accepted"


def loop_tokens(model, prompts, T, patterns, vocab, eos, pad_id=0):
    """The test's own loop: prefill the left-padded batch, read the eager step logits, mask what the oracle does not allow for the bytes
    the row has generated, take the argmax (lowest index on ties), feed it back; a row ends with the end id."""
    B, S, N = len(prompts), max(len(p) for p in prompts), model.config.vocab_size
    ids = torch.full((B, S), pad_id, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    logits = sess.prefill(ids.to(DEV), attention_mask=attn.to(DEV))
    out, done, states = [[] for _ in range(B)], [False] * B, [0] * B
    for t in range(T):
        raw = PO.to_native(logits)
        tok = []
        for b, pattern in enumerate(patterns):
            if done[b]:
                tok.append(0)
                continue
            x = PO.widen(raw[b], "f16")
            if pattern is not None:
                dfa = dfa_of(pattern)
                ok = GO.allowed_ids(dfa, states[b], vocab, eos, N)
                for v in range(N):
                    if v not in ok:
                        x[v] = -np.inf
            tok.append(int(np.argmax(x)))
            out[b].append(tok[-1])
            if tok[-1] == eos:
                done[b] = True
            elif pattern is not None:
                states[b] = GO.walk(dfa, states[b], vocab[tok[-1]])
        if t + 1 < T and not all(done):
            logits = sess.decode_step(torch.tensor(tok, dtype=torch.long, device=DEV)[:, None], greedy=False)
    return out


@pytest.mark.parametrize("pattern", sorted(LANGUAGES))
def test_greedy_generation_equals_the_loop(pattern, tiny16):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = decoder(tiny16)
    T = LANGUAGES[pattern] + 1                                   # the longest word and the end token fit: every row must end accepted
    base = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True))
    assert dec.last_stats["grammar"] is False and dec.last_stats["grammar_state"] is None and dec._session.gr is None
    got = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, grammar=pattern))
    check_row(pattern, got, eos, vocab, dec.last_stats["grammar_state"])
    assert got == loop_tokens(model, [P1], T, [pattern], vocab, eos)[0] and got != base and dec.last_stats["grammar"] is True
    assert "greedy+gr" in dec._session._graphs
    assert got == list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, grammar=dfa_of(pattern), use_graph=False))
    # seeded sampling, on the device and with the host deciding (the launch applied to the logits it gets back): the pattern holds
    for mode in (dict(seed=5), dict(seed=6, top_k=3), dict(seed=7, device_sampler=False), dict(seed=8, top_k=2000)):
        ids = list(dec.generate_ids(P1, max_generated_tokens=T, grammar=pattern, **mode))
        check_row(pattern, ids, eos, vocab, dec.last_stats["grammar_state"])
        if "device_sampler" not in mode and mode.get("top_k", 0) <= 1024:
            assert ids == list(dec.generate_ids(P1, max_generated_tokens=T, grammar=pattern, use_graph=False, **mode))      # graph = eager
    assert "sample+gr" in dec._session._graphs
    # per-row patterns in one batch against the loop; the row without one: the ids of the same call without grammar
    pats = [pattern, None, "[A-D]", "-?[0-9]{1,3}"]
    plain = dec.generate_batch_ids(PROMPTS, max_generated_tokens=5, greedy=True)
    bgot = dec.generate_batch_ids(PROMPTS, max_generated_tokens=5, greedy=True, grammar=pats)
    want = loop_tokens(model, PROMPTS, 5, pats, vocab, eos)
    assert bgot == want and bgot[1] == plain[1]
    for b in (0, 2, 3):
        check_row(pats[b], bgot[b], eos, vocab, dec.last_stats["grammar_state"][b])
    assert dec.last_stats["grammar_state"][1] is None and "rows+gr" in dec._batch_sessions[4][1]._graphs
    # the budget ends inside the pattern
    ids = list(dec.generate_ids(P1, max_generated_tokens=1, greedy=True, grammar=pattern))
    assert ids == got[:1] and dec.last_stats["grammar_state"] == "open"


def test_graph_equals_eager(tiny16):
    dec = decoder(tiny16)
    vocab, eos = tiny_vocab()
    pats = ["(yes|no)", "-?[0-9]{1,3}", None, "[A-D]"]
    kw = dict(max_generated_tokens=5, grammar=pats)
    g = dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=True, **kw)
    assert g == dec.generate_batch_ids(PROMPTS, greedy=True, use_graph=False, **kw)
    skw = dict(kw, top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])
    s = dec.generate_batch_ids(PROMPTS, use_graph=True, **skw)
    states = dec.last_stats["grammar_state"]
    assert s == dec.generate_batch_ids(PROMPTS, use_graph=False, **skw)
    for b in (0, 1, 3):
        check_row(pats[b], s[b], eos, vocab, states[b])
    for mode in (dict(greedy=True), dict(seed=77)):
        one = dict(max_generated_tokens=5, grammar="-?[0-9]{1,3}", **mode)
        assert list(dec.generate_ids(P1, use_graph=True, **one)) == list(dec.generate_ids(P1, use_graph=False, **one))


def test_batch_of_one_equals_generate_ids(tiny16):
    dec = decoder(tiny16)
    kw = dict(max_generated_tokens=5, grammar="-?[0-9]{1,3}")
    assert dec.generate_batch_ids([P1], seed=31, **kw) == [list(dec.generate_ids(P1, seed=31, **kw))]
    assert dec.generate_batch_ids([P1], greedy=True, **kw) == [list(dec.generate_ids(P1, greedy=True, **kw))]
    assert "sample+gr" in dec._session._graphs and "greedy+gr" in dec._session._graphs


def test_row_permutation(tiny16):
    """A row's tokens depend neither on its batch position nor on its neighbours' patterns."""
    prompts = PROMPTS + [[12, 13, 14]]
    seeds, top_k = [101, 202, 303, 404, 505], [100, 1, 100, 30, 100]
    pats = ["(yes|no)", "-?[0-9]{1,3}", None, "[A-D]", "-?[0-9]{1,3}"]
    kw = dict(max_generated_tokens=5)
    plain = decoder(tiny16).generate_batch_ids(prompts, seed=seeds, top_k=top_k, **kw)
    base = decoder(tiny16).generate_batch_ids(prompts, seed=seeds, top_k=top_k, grammar=pats, **kw)
    perm = [3, 0, 4, 2, 1]
    pick = lambda v: [v[i] for i in perm]
    got = decoder(tiny16).generate_batch_ids(pick(prompts), seed=pick(seeds), top_k=pick(top_k), grammar=pick(pats), **kw)
    assert got == pick(base) and base[2] == plain[2] and base[0] != plain[0]


def test_with_penalties_constraints_and_logprobs(tiny16):
    """Penalties, history constraints, the grammar and the log-prob record in one step ("+pen+con+gr+lp"): the pattern holds and the
    record, which reads the masked row, names no masked id - an alternative with a finite log-prob is one the state allowed."""
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = decoder(tiny16)
    pattern = "-?[0-9]{1,3}"
    dfa = dfa_of(pattern)
    kw = dict(max_generated_tokens=5, grammar=pattern, repetition_penalty=1.3, frequency_penalty=0.2, no_repeat_ngram_size=2, logprobs=4)
    for mode in (dict(greedy=True), dict(seed=9)):
        ids = list(dec.generate_ids(P1, **kw, **mode))
        check_row(pattern, ids, eos, vocab, dec.last_stats["grammar_state"])
        rec, state = dec.last_logprobs, 0
        assert len(rec) == len(ids)
        for t, i in enumerate(ids):
            ok = GO.allowed_ids(dfa, state, vocab, eos, cfg.vocab_size)
            assert i in ok and np.isfinite(rec.token_logprobs[t]) and rec.top_ids[t][0] in ok
            assert all(a in ok for a, lp in zip(rec.top_ids[t], rec.top_logprobs[t]) if np.isfinite(lp)), (t, rec.top_ids[t])
            state = GO.walk(dfa, state, vocab[i])
        assert ids == list(decoder(tiny16).generate_ids(P1, use_graph=False, **kw, **mode))      # (a decoder of its own: dec keeps its graphs)
    assert {"greedy+pen+con+gr+lp", "sample+pen+con+gr+lp"} <= set(dec._session._graphs)
    bgot = dec.generate_batch_ids(PROMPTS, seed=[1, 2, 3, 4], **dict(kw, grammar=[pattern, None, "[A-D]", "(yes|no)"]))
    assert "rows+pen+con+gr+lp" in dec._batch_sessions[4][1]._graphs
    for b, p in ((0, pattern), (2, "[A-D]"), (3, "(yes|no)")):
        check_row(p, bgot[b], eos, vocab, dec.last_stats["grammar_state"][b])
        state, rec = 0, dec.last_logprobs[b]
        for t, i in enumerate(bgot[b]):
            ok = GO.allowed_ids(dfa_of(p), state, vocab, eos, cfg.vocab_size)
            assert all(a in ok for a, lp in zip(rec.top_ids[t], rec.top_logprobs[t]) if np.isfinite(lp))
            state = GO.walk(dfa_of(p), state, vocab[i])


def test_capture_walks_nothing(tiny16):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    B = 3
    prompts = [[5, 9, 200], [44, 3, 1], [100, 101, 102]]
    for mode in ("rows", "greedy"):
        sess = DecodeSession(model, B, 64, use_graph=True)
        assert sess.gr is None
        with pytest.raises(ValueError):
            sess.arm_grammar(["[a-d]*", None, "(yes|no| )*"], eos)          # no byte table yet
        assert sess.arm_grammar([None] * 3, eos) is False and sess.gr is None
        assert sess.arm_grammar(["[a-d]*", None, "(yes|no| )*"], eos, TOKEN_BYTES()) and sess.gr is not None
        sess.arm_rows([(1, 0.8, 1.0)] * B, [1, 2, 3], [12] * B, eos)
        logits = sess.grammar_first(sess.prefill(torch.tensor(prompts)), rows=mode == "rows")
        if mode == "rows":
            sess.sample_rows_first(logits)
        else:
            sess.tok.copy_(logits.argmax(-1, keepdim=True))
        first = sess.tok.view(-1).tolist()
        kw = dict(greedy=mode == "greedy", rows=mode == "rows", gr=True)
        sess.capture(**kw)
        torch.cuda.synchronize()
        assert sess.gr.states() == [0, 0, 0] and sess.gr.ticket.tolist() == [0] * B, "the capture's warm-up runs walked a state"
        sess.decode_step(**kw)
        torch.cuda.synchronize()
        assert mode + "+gr" in sess._graphs
        want = [GO.walk(dfa_of("[a-d]*"), 0, vocab[first[0]]), 0, GO.walk(dfa_of("(yes|no| )*"), 0, vocab[first[2]])]
        assert sess.gr.states() == want and want[0] >= 0 and want[2] >= 0


# launches of the same calls on the commit before this feature (tiny fp16 model, T = 9): generate_ids greedy / sampled and
# generate_batch_ids greedy / sampled with use_graph=False; generate_ids greedy and generate_batch_ids sampled on fresh graph sessions.
# The calls are test_constraints_gpu.py's, which asserts the same numbers on that commit
PARENT_EAGER_LAUNCHES = [125, 126, 172, 172]
PARENT_GRAPH_LAUNCHES = [47, 64]


def test_launch_accounting(tiny16):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    p = [17, 3, 99, 250]
    T = 9
    # 400 bytes before the pattern is complete: more than T tokens hold, so the end id is never allowed and every row generates T tokens
    gr = dict(grammar="[a-d0-9 ,]{400}")

    def launches(fn):
        before = _lib.launch_count()
        fn()
        torch.cuda.synchronize()
        return _lib.launch_count() - before

    warm = ChatGLMDecoder(cfg, model)                            # build every lazy layout the steps read before anything is counted
    list(warm.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    warm.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    # eager steps: a constrained token costs exactly one launch more (T - 1 steps and the first token).  A grammar needs the end id; the
    # unconstrained leg runs without one so that it generates T tokens too (the end id changes no launch)
    gens = (lambda d, **k: list(d.generate_ids(p, max_generated_tokens=T, use_graph=False, **k)),
            lambda d, **k: d.generate_batch_ids(PROMPTS, max_generated_tokens=T, use_graph=False, **k))
    offs = []
    for n, gen in enumerate(gens):
        for mode in (dict(greedy=True), dict(seed=3)):
            dec = ChatGLMDecoder(cfg, model)
            off = launches(lambda: gen(dec, ignore_eos=True, **mode))
            assert dec.last_stats["grammar"] is False
            con = decoder(tiny16)
            on = launches(lambda: gen(con, **mode, **gr))
            assert con.last_stats["grammar"] is True and con.last_stats["generated"] == (T if n == 0 else [T] * 4)
            assert con.last_stats["grammar_state"] == ("open" if n == 0 else ["open"] * 4)
            assert on == off + T, (on, off, mode)
            offs.append(off)
    # every new argument at its default: exactly the launches of the commit before the grammar (counted there, same calls)
    assert offs == PARENT_EAGER_LAUNCHES, offs
    # graphs: an unconstrained generation on a session that holds "+gr" graphs issues what it issues on a fresh session
    fresh = launches(lambda: list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    dec = decoder(tiny16)
    list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, **gr))
    assert launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))) == fresh
    assert set(dec._session._graphs) == {"greedy+gr", "greedy"}
    bfresh = launches(lambda: ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    assert [fresh, bfresh] == PARENT_GRAPH_LAUNCHES, (fresh, bfresh)
    bdec = decoder(tiny16)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, **gr)
    # (a fresh capture of "rows" on both sides: the batched step bakes the stop id in, and this call has none)
    assert launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True)) == bfresh
    # both graphs captured under the same stop id: only the first token's launch is extra, the steps are replays
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, **gr)
    assert {"rows", "rows+gr"} <= set(bdec._batch_sessions[4][1]._graphs)
    again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1))
    gr_again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, **gr))
    assert bdec.last_stats["generated"] == [T] * 4 and gr_again == again + 1
    # with grammar=None nothing is armed or allocated
    d = decoder(tiny16)
    list(d.generate_ids(p, max_generated_tokens=T, greedy=True, grammar=None))
    d.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, grammar=[None] * 4)
    assert d._session.gr is None and d._batch_sessions[4][1].gr is None and d.last_stats["grammar"] is False

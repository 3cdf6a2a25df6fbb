"""JSON-constrained generation on the GPU: ``qlinear_pda_mask`` (csrc/pda_mask.hip) through ``fused_ops`` / ctypes against the oracle
(tests/_pda_oracle.py) - logits as integer bit patterns, state, depth, every stack byte and the tickets all equal - over a scripted
sequence that takes a JSON row from depth 0 to max_depth and back (eager and as a replayed graph: the configuration advances exactly once
per replay), a lifted DFA row against ``qlinear_grammar_mask`` itself, corrupt device state, a random table at the cap, and the captured
"+pda" steps of ``ChatGLMDecoder.generate_ids`` / ``generate_batch_ids`` against a loop written here and against the launch counter."""
import functools
import random

import numpy as np
import pytest
import torch

import _grammar_oracle as GO
import _pda_oracle as PD
import _penalty_oracle as PO
import test_grammar_gpu as TGG
import test_pda_cpu as TPC
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd import grammar as G
from chatglm_q_amd.decoder import ChatGLMDecoder, DecodeSession
from test_model_cpu import build as build_tiny

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIN = fused_ops.BatchRows.FINISHED
bits_of = TGG.bits_of
N = 700                                                         # three workgroups per row, the last one partial: 2 x 256 + 188
N_TOK = 697                                                     # ... and three ids past the vocabulary's table
PIECES = (b'{"', b'":', b'"}]}', b"[[[", b"]]", b"],[", b"1.5e-3,", b"", b"[" * 33, b"[" * 32, b"\xc3", b"\xa9", b"\xe2", b"\x82", b"\xac", b"BC", b"AB", b"[]")
SINGLES = b'[]{},:"0123456789-+.eEtrufalsn\\/b \n\t\rABCDxyz'


@functools.lru_cache(maxsize=None)
def vocab700():
    vocab = GO.make_vocab(N_TOK, seed=4, singles=SINGLES, alphabet=b'[]{},:"01-.eatrue ABCD', extra=PIECES)
    assert all(vocab.count(t) >= 1 for t in PIECES) and len(vocab) == N_TOK
    return vocab


@functools.lru_cache(maxsize=None)
def token_table():
    return G.token_byte_table(vocab700())


def tid(piece):
    return vocab700().index(piece)


JSON4 = TPC.J(True, max_depth=4)
LIFTED = G.BytePDA.from_dfa(G.compile_regex("[A-D]+"))
# the JSON row: depth 0 -> 4 (max_depth), the mask there refuses every opener, a piece that pops three levels below the walk's own
# pushes, pieces that push and pop inside one token, a number ended by its comma, back to depth 0, the end id, then a byte that kills it
SCRIPT = [None, b"[", b'{"', b"a", b'":', b"[", b'{"', b"b", b'":', b'"', b"\xc3", b"\xa9", b'"}]}', b",", b"[[[", b"]]", b"],[", b"1.5e-3,", b"1", b"]]",
          b" ", "eos", b"x"]
DFA_FEED = [None, b"A", b"BC", b"", b"D", "past", b"A", b"B", "eos", b"C", b"D", b"AB", b"A", b"A", b"B", b"C", b"D", b"A", b"B", b"C", b"D", b"x", b"A"]


def script_ids():
    """Per launch the fed ids of the four rows: no grammar, finished (its bit set: untouched whatever is fed), the lifted DFA, JSON."""
    vocab = vocab700()
    eos = [i for i, t in enumerate(vocab) if not t][1]
    feeds = []
    for js, d in zip(SCRIPT, DFA_FEED):
        if js is None:
            feeds.append(None)
            continue
        one = lambda t: eos if t == "eos" else N_TOK + 1 if t == "past" else vocab.index(t)
        feeds.append([5, vocab.index(b"["), one(d), one(js)])
    return eos, feeds


def fresh_rows(eos, which=(0, 1, 2, 3)):
    rows = [PD.new_row(None, eos, N), PD.new_row(JSON4, eos, N), PD.new_row(LIFTED, eos, N), PD.new_row(JSON4, eos, N)]
    return [rows[i] for i in which]


@functools.lru_cache(maxsize=None)
def script_reference(which=(0, 1, 2, 3)):
    """The oracle over the whole script, once: per launch the masked columns of every row and the rows behind the launch."""
    eos, feeds = script_ids()
    rows = fresh_rows(eos, which)
    finished = [[0, FIN if i == 1 else 0] for i in which]
    out = []
    for fed in feeds:
        marks = np.zeros((len(rows), N), dtype=np.uint32)
        PD.launch(marks, "f32", rows, vocab700(), None if fed is None else [fed[i] for i in which], finished)
        out.append((marks == PD.NEG_INF["f32"], [dict(r, stack=list(r["stack"])) for r in rows]))
    json_row = which.index(3)
    depths = [rows_after[json_row]["depth"] for _, rows_after in out]
    assert max(depths) == 4 and depths[8] == 4 and depths[19] == 0 and out[-1][1][json_row]["state"] == -1 and out[-2][1][json_row]["state"] >= 0
    at4 = out[8][0][json_row]                                   # at max_depth every opener is refused, single or inside a piece
    assert all(at4[tid(t)] for t in (b"[", b"{", b"[[[", b'{"')) and not at4[tid(b'"')] and not at4[tid(b"1")]
    assert not out[19][0][json_row][eos] and out[18][0][json_row][eos]       # the end id exactly with an empty stack in an accepting state
    assert out[0][0][json_row][tid(b"[" * 33)] and out[0][0][json_row][tid(b"[[[")] == False and out[1][0][json_row][tid(b"[[[")] == False
    return eos, feeds, finished, out


def run_script(dt, which, graph, ld_extra):
    eos, feeds, finished, ref = script_reference(which)
    B = len(which)
    rows = fresh_rows(eos, which)
    st = fused_ops.PdaState(B, token_table(), DEV).arm([r["pda"] for r in rows], [r["eos"] for r in rows])
    rs_t = torch.tensor(finished, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(len(which) * 100 + ld_extra)
    buf = torch.zeros(B, N + ld_extra, dtype=PO.DTYPES[dt], device=DEV)
    view = buf[:, :N] if ld_extra else buf
    tok = torch.zeros(B, dtype=torch.int64, device=DEV)
    body = lambda: fused_ops.pda_mask(view, st, tok, rs_t)
    g = None
    for step, fed in enumerate(feeds):
        host = (torch.randn(B, N + ld_extra, generator=gen) * 4).to(PO.DTYPES[dt])
        want = bits_of(host)
        buf.copy_(host)
        before = _lib.launch_count()
        if fed is None:
            fused_ops.pda_mask(view, st, None, rs_t)
        else:
            tok.copy_(torch.tensor([fed[i] for i in which], dtype=torch.int64))
            if graph and g is None:                             # capture one launch; the warm-up and the capture must not move the rows
                saved = [t.clone() for t in st.tensors()]
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    body()
                torch.cuda.current_stream().wait_stream(side)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    body()
                for dst, src in zip(st.tensors(), saved):
                    dst.copy_(src)
                buf.copy_(host)
                before = _lib.launch_count()
            g.replay() if graph else body()
        torch.cuda.synchronize()
        if not graph:
            assert _lib.launch_count() == before + 1
        masked, rows_after = ref[step]
        want[:, :N][masked] = PD.NEG_INF[dt]
        got = bits_of(buf)
        assert np.array_equal(got, want), (dt, step, np.argwhere(got != want)[:8])
        PD.assert_rows(st, rows_after)                          # exactly one advance per launch / replay, every stack byte
    assert rs_t.tolist() == finished


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
def test_scripted_sequence(dt, graph):
    run_script(dt, (0, 1, 2, 3), graph, ld_extra=0 if dt == "f32" else 9)        # (a logits row stride larger than N)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_scripted_sequence_batch_1(graph):
    run_script("f16", (3,), graph, ld_extra=0)


def test_lifted_dfa_row_equals_the_dfa_kernel():
    """The same DFA, the same fed ids: ``qlinear_pda_mask`` on the lifted automaton against ``qlinear_grammar_mask`` - the reference here
    is the existing kernel - logits bit for bit and the state after every launch."""
    eos, feeds = script_ids()
    dfa = G.compile_regex("[A-D]+")
    pst = fused_ops.PdaState(2, token_table(), DEV).arm([dfa, dfa], [eos, -1])
    gst = fused_ops.GrammarState(2, token_table(), DEV).arm([dfa, dfa], [eos, -1])
    gen = torch.Generator().manual_seed(3)
    for fed in feeds:
        host = (torch.randn(2, N + 3, generator=gen) * 4).to(torch.float16)
        a, b = host.to(DEV), host.to(DEV)
        tok = None if fed is None else torch.tensor([fed[2], fed[2]], dtype=torch.int64, device=DEV)
        fused_ops.pda_mask(a[:, :N], pst, tok)
        fused_ops.grammar_mask(b[:, :N], gst, tok)
        torch.cuda.synchronize()
        assert np.array_equal(bits_of(a), bits_of(b)) and pst.states() == gst.states() and pst.depth.tolist() == [0, 0]
    assert pst.states() == [-1, -1] and pst.ticket.tolist() == [0, 0]


CORRUPT = {
    # name: (what the test writes into the row behind arm, the fed piece)
    "depth_65": (dict(depth=65), b"1"),
    "depth_minus_1": (dict(depth=-1), b"1"),
    "top_symbol_3": (dict(depth=2, stack=[1, 3]), b"1"),
    "symbol_3_beneath": (dict(state="after", depth=3, stack=[1, 3, 1]), b"]]"),
    "n_syms_9": (dict(depth=2, stack=[1, 2], n_syms=9), b"1"),
    "n_syms_minus_4": (dict(n_syms=-4), b"1"),
    "max_depth_1000": (dict(state="array-open", depth=4, stack=[1, 1, 1, 1], max_depth=1000), b"[[["),
    "max_depth_minus_1": (dict(max_depth=-1), b"[]"),
    "state_5000": (dict(state=5000), b"1"),
    "n_states_100000": (dict(n_states=100000), b"[[["),
    "valid": (dict(state="array-open", depth=1, stack=[1]), b"[[["),
}


def test_corrupt_device_state():
    """Rows the test corrupts after ``arm``: each gives the oracle's result - dead or clamped, never an index out of range - and the
    rows without a grammar, the columns past N and the other rows' stacks keep every bit."""
    vocab = vocab700()
    eos = [i for i, t in enumerate(vocab) if not t][1]
    names = sorted(CORRUPT)
    states = {"after": 5, "array-open": 1}                      # json_grammar numbers its states in the order it creates them
    assert JSON4.accept[5] and JSON4.step(JSON4.start, b"[") == (1, (1,))
    rows, tok = [PD.new_row(None, eos, N)], [7]
    for name in names:
        spec, fed = CORRUPT[name]
        r = PD.new_row(JSON4, eos, N)
        for k, v in spec.items():
            if k == "stack":
                r["stack"][:len(v)] = v
            else:
                r[k] = states.get(v, v) if k == "state" else v
        rows.append(r)
        tok.append(vocab.index(fed))
    B = len(rows)
    st = PD.device_rows(fused_ops.PdaState(B, token_table(), DEV).arm([r["pda"] for r in rows], [r["eos"] for r in rows]), rows)
    host = (torch.randn(B, N + 5, generator=torch.Generator().manual_seed(1)) * 4).to(torch.bfloat16)
    want = bits_of(host)
    buf = host.to(DEV)
    fused_ops.pda_mask(buf[:, :N], st, torch.tensor(tok, dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    PD.launch(want, "bf16", rows, vocab, tok)
    got = bits_of(buf)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]
    PD.assert_rows(st, rows)
    after = {name: rows[1 + i] for i, name in enumerate(names)}
    for name in ("depth_65", "depth_minus_1", "top_symbol_3", "symbol_3_beneath", "state_5000", "max_depth_minus_1"):
        assert after[name]["state"] == -1, name
    assert after["valid"]["depth"] == 4 and after["max_depth_1000"]["depth"] == 7 and after["n_states_100000"]["depth"] == 3
    assert after["n_syms_minus_4"]["state"] >= 0                 # no symbols, no pushes: a number is still a number
    deep = want[1 + names.index("max_depth_1000")]              # depth 7 of 64: only the window rule refuses 33 openers in one token
    assert deep[vocab.index(b"[" * 32)] != PD.NEG_INF["bf16"] and deep[vocab.index(b"[" * 33)] == PD.NEG_INF["bf16"]


def test_a_random_table_at_the_cap():
    """32 states x 4 stack tops x 128 byte classes = 16 384 entries of random moves - next states in and out of range, every op, every
    symbol - from random configurations: whatever the table says, the kernel's walk is the oracle's."""
    rng = np.random.default_rng(16384)
    table = (rng.integers(0, 36, (32, 4, 128)) | rng.choice([0, 0, 0, 1, 1, 2, 2, 3], (32, 4, 128)) << 12 | rng.integers(0, 4, (32, 4, 128)) << 14)
    pda = G.BytePDA(np.arange(256) % 128, table.astype(np.uint16), rng.integers(0, 2, 32), 3, 64)
    assert pda.table.size == fused_ops.GRAMMAR_TABLE_MAX == pda.n_states * (pda.n_syms + 1) * pda.n_classes
    vocab, r = vocab700(), random.Random(5)
    rows, walked = [], 0
    for b in range(6):
        row = PD.new_row(pda, r.choice([-1, 3, N - 1]), N)
        row["state"], row["depth"] = r.randrange(32), r.choice([0, 1, 5, 33, 64])
        row["stack"] = [r.randrange(1, 4) for _ in range(64)]
        rows.append(row)
    st = PD.device_rows(fused_ops.PdaState(6, token_table(), DEV).arm([pda] * 6, [row["eos"] for row in rows]), rows)
    for step in range(3):
        survivors = [sorted(PD.allowed_ids(PD.Machine(row), None if row["state"] < 0 else (row["state"], row["stack"][:row["depth"]]), vocab, -1, N))
                     for row in rows]
        tok = [r.choice(s) if s and r.random() < 0.8 else r.randrange(N_TOK) for s in survivors]
        walked += sum(1 for b, s in enumerate(survivors) if tok[b] in s and len(vocab[tok[b]]) > 1)
        host = (torch.randn(6, N, generator=torch.Generator().manual_seed(step)) * 4).to(torch.float16)
        want = bits_of(host)
        buf = host.to(DEV)
        fused_ops.pda_mask(buf, st, torch.tensor(tok, dtype=torch.int64, device=DEV))
        torch.cuda.synchronize()
        PD.launch(want, "f16", rows, vocab, tok)
        assert np.array_equal(bits_of(buf), want), step
        PD.assert_rows(st, rows)
    assert walked >= 4                                          # (the random moves leave something to walk)


def test_argument_errors_and_no_launch():
    lib = _lib.get_lib()
    B = 2
    st = fused_ops.PdaState(B, token_table(), DEV).arm([LIFTED, LIFTED], [-1, -1])
    lg = torch.zeros(B, N, dtype=torch.float16, device=DEV)
    f16 = _lib.dtype_code(torch.float16)

    def call(logits=lg.data_ptr(), b=B, n=N, ldl=N, off=st.tok_off.data_ptr(), data=st.tok_bytes.data_ptr(), n_tok=st.n_tok, n_bytes=st.n_bytes,
             class_of=st.class_of.data_ptr(), table=st.table.data_ptr(), accept=st.accept.data_ptr(), cfg=st.cfg.data_ptr(),
             state=st.state.data_ptr(), depth=st.depth.data_ptr(), stack=st.stack.data_ptr(), ticket=st.ticket.data_ptr(), dtype=f16):
        return lib.qlinear_pda_mask(logits, b, n, ldl, off, data, n_tok, n_bytes, class_of, table, accept, cfg, state, depth, stack, ticket, None,
                                    None, dtype, _lib.stream_ptr(lg.device))
    before = _lib.launch_count()
    for missing in ("logits", "off", "data", "class_of", "table", "accept", "cfg", "state", "depth", "stack", "ticket"):
        assert call(**{missing: 0}) == -1                        # QL_ERR_NULL_POINTER
    assert call(ldl=N - 1) == -2 and call(n=0) == -2 and call(n_tok=0) == -2 and call(n_bytes=-1) == -2 and call(b=65536) == -2
    assert call(table=st.table.data_ptr() + 2) == -5 and call(depth=st.depth.data_ptr() + 2) == -5      # QL_ERR_MISALIGNED
    assert call(dtype=99) == -3                                 # QL_ERR_BAD_DTYPE
    assert call(b=0, logits=0) == 0                             # QL_OK, no launch
    assert _lib.launch_count() == before
    torch.cuda.synchronize()
    assert not lg.any() and st.states() == [0, 0]               # nothing ran
    assert call() == 0 and _lib.launch_count() == before + 1
    torch.cuda.synchronize()
    allowed = [i for i, t in enumerate(vocab700()) if t and all(v in b"ABCD" for v in t)]
    assert allowed and (~torch.isinf(lg[0])).nonzero().view(-1).tolist() == allowed == (~torch.isinf(lg[1])).nonzero().view(-1).tolist()
    with pytest.raises(ValueError):
        fused_ops.pda_mask(lg[:1], st)
    with pytest.raises(ValueError):
        fused_ops.pda_mask(lg.cpu(), st)


# ---- the session and the API ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny16():
    return build_tiny("f16", DEV)


P1 = TGG.P1
PROMPTS = TGG.PROMPTS


@functools.lru_cache(maxsize=None)
def tiny_vocab(n=256):
    vocab = TPC.pda_vocab(n, seed=11)
    eos = [i for i, t in enumerate(vocab) if not t][1]
    assert eos not in P1 and all(eos not in q for q in PROMPTS)
    return vocab, eos


@functools.lru_cache(maxsize=None)
def TOKEN_BYTES():
    return G.token_byte_table(tiny_vocab()[0])


def decoder(tiny16, **kw):
    model, cfg = tiny16
    return ChatGLMDecoder(cfg, model, eos_token_id=tiny_vocab(cfg.vocab_size)[1], token_bytes=TOKEN_BYTES(), **kw)


def as_pda(g):
    return None if g is None else g if isinstance(g, G.BytePDA) else G.BytePDA.from_dfa(TGG.dfa_of(g))


def loop_tokens(model, prompts, T, grammars, vocab, eos, pad_id=0):
    """The test's own loop: prefill the left-padded batch, read the eager step logits, mask what the ORACLE does not allow for the
    configuration the row's generated bytes lead to, take the argmax (lowest index on ties), feed it back; a row ends with the end id."""
    B, S, NV = len(prompts), max(len(p) for p in prompts), model.config.vocab_size
    ids = torch.full((B, S), pad_id, dtype=torch.long)
    attn = torch.zeros(B, S, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, S - len(p):] = torch.tensor(p)
        attn[b, S - len(p):] = 1
    sess = DecodeSession(model, B, -(-(S + T) // 64) * 64, use_graph=False)
    logits = sess.prefill(ids.to(DEV), attention_mask=attn.to(DEV))
    machines = [None if g is None else PD.Machine(PD.new_row(as_pda(g), eos, NV)) for g in grammars]
    out, done, configs = [[] for _ in range(B)], [False] * B, [(0, []) for _ in range(B)]
    for t in range(T):
        raw = PO.to_native(logits)
        tok = []
        for b, m in enumerate(machines):
            if done[b]:
                tok.append(0)
                continue
            x = PO.widen(raw[b], "f16")
            if m is not None:
                ok = PD.allowed_ids(m, configs[b], vocab, eos, NV)
                for v in range(NV):
                    if v not in ok:
                        x[v] = -np.inf
            tok.append(int(np.argmax(x)))
            out[b].append(tok[-1])
            if tok[-1] == eos:
                done[b] = True
            elif m is not None:
                configs[b] = m.walk(configs[b][0], configs[b][1], vocab[tok[-1]])
        if t + 1 < T and not all(done):
            logits = sess.decode_step(torch.tensor(tok, dtype=torch.long, device=DEV)[:, None], greedy=False)
    return out


def check(g, ids, eos, vocab, state):
    if isinstance(g, G.BytePDA):
        return TPC.check_json_row(g, ids, eos, vocab, state)
    TGG.check_row(g, ids, eos, vocab, state)
    return state


def test_generation_equals_the_loop(tiny16):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = decoder(tiny16)
    js, T = TPC.J(True, max_depth=4), 12
    base = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True))
    assert dec.last_stats["grammar"] is False and dec._session.gr is None and dec._session.pda is None
    got = list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, grammar=js))
    check(js, got, eos, vocab, dec.last_stats["grammar_state"])
    assert got == loop_tokens(model, [P1], T, [js], vocab, eos)[0] and got != base and dec.last_stats["grammar"] is True
    assert "greedy+pda" in dec._session._graphs and "greedy+gr" not in dec._session._graphs and dec._session.gr is None
    assert got == list(dec.generate_ids(P1, max_generated_tokens=T, greedy=True, grammar=js, use_graph=False))
    seen = set()
    for mode in (dict(seed=5), dict(seed=6, top_k=3), dict(seed=7, device_sampler=False), dict(seed=8, top_k=2000)):
        ids = list(dec.generate_ids(P1, max_generated_tokens=T, grammar=js, **mode))
        seen.add(check(js, ids, eos, vocab, dec.last_stats["grammar_state"]))
        if "device_sampler" not in mode and mode.get("top_k", 0) <= 1024:
            assert ids == list(dec.generate_ids(P1, max_generated_tokens=T, grammar=js, use_graph=False, **mode))      # graph = eager
    assert "sample+pda" in dec._session._graphs
    # mixed rows in one batch against the loop; the row without a grammar: the ids of the same call without
    grammars = [js, None, "[A-D]", TPC.J(False, "array", 3)]
    plain = dec.generate_batch_ids(PROMPTS, max_generated_tokens=8, greedy=True)
    bgot = dec.generate_batch_ids(PROMPTS, max_generated_tokens=8, greedy=True, grammar=grammars)
    states = dec.last_stats["grammar_state"]
    assert bgot == loop_tokens(model, PROMPTS, 8, grammars, vocab, eos) and bgot[1] == plain[1] and states[1] is None
    for b in (0, 2, 3):
        seen.add(check(grammars[b], bgot[b], eos, vocab, states[b]))
    sess = dec._batch_sessions[4][1]
    assert "rows+pda" in sess._graphs and "rows+gr" not in sess._graphs
    assert bgot == dec.generate_batch_ids(PROMPTS, max_generated_tokens=8, greedy=True, grammar=grammars, use_graph=False)
    skw = dict(max_generated_tokens=8, grammar=grammars, top_k=[7, 100, 1024, 1], top_p=[0.8, 0.3, 1.0, 0.8], temperature=[1.0, 0.5, 1.7, 1.0], seed=[5, 6, 7, 8])
    s = dec.generate_batch_ids(PROMPTS, use_graph=True, **skw)
    states = dec.last_stats["grammar_state"]
    assert s == dec.generate_batch_ids(PROMPTS, use_graph=False, **skw)
    for b in (0, 2, 3):
        seen.add(check(grammars[b], s[b], eos, vocab, states[b]))
    # the budget ends inside the document
    ids = list(dec.generate_ids(P1, max_generated_tokens=1, greedy=True, grammar=js))
    assert ids == got[:1] and dec.last_stats["grammar_state"] in ("open",) and "accepted" in seen


def test_with_penalties_constraints_and_logprobs(tiny16):
    """Penalties, history constraints, the pushdown automaton and the log-prob record in one step ("+pen+con+pda+lp"): the grammar holds
    and the record, which reads the masked row, names no masked id."""
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = decoder(tiny16)
    js = TPC.J(True, max_depth=4)
    m = PD.Machine(PD.new_row(js, eos, cfg.vocab_size))
    kw = dict(max_generated_tokens=8, grammar=js, repetition_penalty=1.3, frequency_penalty=0.2, no_repeat_ngram_size=2, logprobs=4)
    for mode in (dict(greedy=True), dict(seed=9)):
        ids = list(dec.generate_ids(P1, **kw, **mode))
        check(js, ids, eos, vocab, dec.last_stats["grammar_state"])
        rec, config = dec.last_logprobs, (0, [])
        assert len(rec) == len(ids)
        for t, i in enumerate(ids):
            ok = PD.allowed_ids(m, config, vocab, eos, cfg.vocab_size)
            assert i in ok and np.isfinite(rec.token_logprobs[t]) and rec.top_ids[t][0] in ok
            assert all(a in ok for a, lp in zip(rec.top_ids[t], rec.top_logprobs[t]) if np.isfinite(lp)), (t, rec.top_ids[t])
            config = config if i == eos else m.walk(config[0], config[1], vocab[i])
        assert ids == list(decoder(tiny16).generate_ids(P1, use_graph=False, **kw, **mode))
    assert {"greedy+pen+con+pda+lp", "sample+pen+con+pda+lp"} <= set(dec._session._graphs)
    grammars = [js, None, "[A-D]", js]
    bgot = dec.generate_batch_ids(PROMPTS, seed=[1, 2, 3, 4], **dict(kw, grammar=grammars))
    assert "rows+pen+con+pda+lp" in dec._batch_sessions[4][1]._graphs
    for b in (0, 2, 3):
        check(grammars[b], bgot[b], eos, vocab, dec.last_stats["grammar_state"][b])


def test_capture_walks_nothing(tiny16):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    js = TPC.J(True, max_depth=4)
    sess = DecodeSession(model, 3, 64, use_graph=True)
    with pytest.raises(ValueError):
        sess.arm_grammar([js, None, "[A-D]+"], eos)             # no byte table yet
    assert sess.arm_grammar([None] * 3, eos) is False and sess.pda is None and sess.gr is None
    assert sess.arm_grammar(["[A-D]+", None, None], eos, TOKEN_BYTES()) and sess.gr is not None and sess.pda is None and not sess.pda_armed
    assert sess.arm_grammar([js, None, "[A-D]+"], eos, TOKEN_BYTES()) and sess.pda_armed and not sess.gr.active
    sess.arm_rows([(1, 0.8, 1.0)] * 3, [1, 2, 3], [12] * 3, eos)
    logits = sess.pda_first(sess.prefill(torch.tensor([[5, 9, 200], [44, 3, 1], [100, 101, 102]])), rows=True)
    sess.sample_rows_first(logits)
    first = sess.tok.view(-1).tolist()
    sess.capture(greedy=False, rows=True, pda=True)
    torch.cuda.synchronize()
    assert sess.pda.configs() == [(0, ())] * 3 and sess.pda.ticket.tolist() == [0] * 3, "the capture's warm-up runs walked a configuration"
    sess.decode_step(greedy=False, rows=True, pda=True)
    torch.cuda.synchronize()
    assert "rows+pda" in sess._graphs
    want = [js.step(js.start, vocab[first[0]]), (0, ()), LIFTED.step(LIFTED.start, vocab[first[2]])]
    assert sess.pda.configs() == want and want[0] is not None and want[2] is not None


def test_launch_accounting(tiny16, monkeypatch):
    model, cfg = tiny16
    vocab, eos = tiny_vocab(cfg.vocab_size)
    p, T = [17, 3, 99, 250], 9
    # 400 bytes before the language is complete: the end id is never allowed and every row generates T tokens.  As a BytePDA the call takes
    # the pushdown launch, as a pattern the DFA launch
    pattern = "[a-d0-9 ,]{400}"
    lifted = G.BytePDA.from_dfa(G.compile_regex(pattern))
    calls = {"pda": 0, "gr": 0}
    real_pda, real_gr = fused_ops.pda_mask, fused_ops.grammar_mask
    monkeypatch.setattr(fused_ops, "pda_mask", lambda *a, **k: (calls.__setitem__("pda", calls["pda"] + 1), real_pda(*a, **k))[1])
    monkeypatch.setattr(fused_ops, "grammar_mask", lambda *a, **k: (calls.__setitem__("gr", calls["gr"] + 1), real_gr(*a, **k))[1])

    def launches(fn):
        before = _lib.launch_count()
        fn()
        torch.cuda.synchronize()
        return _lib.launch_count() - before

    warm = ChatGLMDecoder(cfg, model)
    list(warm.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))
    warm.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, ignore_eos=True)
    gens = (lambda d, **k: list(d.generate_ids(p, max_generated_tokens=T, use_graph=False, **k)),
            lambda d, **k: d.generate_batch_ids(PROMPTS, max_generated_tokens=T, use_graph=False, **k))
    offs = []
    for n, gen in enumerate(gens):
        for mode in (dict(greedy=True), dict(seed=3)):
            dec = ChatGLMDecoder(cfg, model)
            calls.update(pda=0, gr=0)
            off = launches(lambda: gen(dec, ignore_eos=True, **mode))
            assert dec.last_stats["grammar"] is False and calls == {"pda": 0, "gr": 0}
            con = decoder(tiny16)
            on = launches(lambda: gen(con, grammar=lifted, **mode))
            assert con.last_stats["grammar"] is True and con.last_stats["generated"] == (T if n == 0 else [T] * 4)
            assert on == off + T, (on, off, mode)               # a "+pda" token: exactly one launch more
            assert calls == {"pda": T, "gr": 0}
            calls.update(pda=0, gr=0)
            dfa_on = launches(lambda: gen(con, grammar=pattern, **mode))
            assert dfa_on == off + T and calls == {"pda": 0, "gr": T}        # a DFA-only call: the DFA launch, never the pushdown one
            offs.append(off)
    assert offs == TGG.PARENT_EAGER_LAUNCHES, offs              # without a grammar: what the calls issued before
    fresh = launches(lambda: list(ChatGLMDecoder(cfg, model).generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True)))
    dec = decoder(tiny16)
    list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, grammar=lifted))
    assert launches(lambda: list(dec.generate_ids(p, max_generated_tokens=T, greedy=True, ignore_eos=True))) == fresh
    assert set(dec._session._graphs) == {"greedy+pda", "greedy"}
    bfresh = launches(lambda: ChatGLMDecoder(cfg, model).generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, ignore_eos=True))
    assert [fresh, bfresh] == TGG.PARENT_GRAPH_LAUNCHES, (fresh, bfresh)
    bdec = decoder(tiny16)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1)
    bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, grammar=lifted)
    assert {"rows", "rows+pda"} <= set(bdec._batch_sessions[4][1]._graphs)
    again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1))
    pda_again = launches(lambda: bdec.generate_batch_ids(PROMPTS, max_generated_tokens=T, seed=1, grammar=lifted))
    assert bdec.last_stats["generated"] == [T] * 4 and pda_again == again + 1       # replays: only the first token's launch is extra
    d = decoder(tiny16)
    list(d.generate_ids(p, max_generated_tokens=T, greedy=True, grammar=None))
    d.generate_batch_ids(PROMPTS, max_generated_tokens=T, greedy=True, grammar=[None] * 4)
    assert d._session.pda is None and d._batch_sessions[4][1].pda is None and d._session.gr is None and d.last_stats["grammar"] is False

"""JSON-constrained generation, CPU branch: ``grammar.json_grammar`` against Python's ``json`` on random nested values and on every
one-byte mutation of their documents, the depth bound, ``BytePDA.from_dfa`` against ``ByteDFA``, the caps, the host form of
``fused_ops.pda_mask`` against the oracle (tests/_pda_oracle.py) bit for bit, the declarations, and ``ChatGLMDecoder.generate_ids`` /
``generate_batch_ids`` with a ``BytePDA`` on the CPU tiny model over a synthetic vocabulary.  The GPU twin (the HIP kernel, the captured
"+pda" steps) is test_pda_gpu.py."""
import functools
import itertools
import json
import os
import random
import re

import numpy as np
import pytest
import torch

import _pda_oracle as PD
import test_grammar_cpu as TG
from chatglm_q_amd import _lib, fused_ops
from chatglm_q_amd import grammar as G
from chatglm_q_amd.decoder import ChatGLMDecoder
from test_model_cpu import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32}
to_bits = TG.to_bits


# ---- json_grammar against Python's json ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def J(whitespace=False, root="value", max_depth=16):
    return G.json_grammar(root=root, whitespace=whitespace, max_depth=max_depth)


def strict_loads(doc: bytes):
    """(accepted, value) by Python's parser made strict: NaN / Infinity / -Infinity rejected (parse_constant raises).  One category is
    decided by RFC 8259 against Python's parser and excluded exactly: bytes that are not well-formed UTF-8 (section 8.1 requires UTF-8;
    ``json.loads`` on bytes guesses UTF-16 / UTF-32 from NUL bytes, accepts a byte order mark and decodes with "surrogatepass") - the
    document is decoded as strict UTF-8 first and counts as rejected when that fails."""
    def constant(name):
        raise ValueError(name)
    try:
        return True, json.loads(doc.decode("utf-8"), parse_constant=constant)
    except (ValueError, RecursionError):                        # (UnicodeDecodeError and JSONDecodeError are ValueErrors)
        return False, None


def nesting(v):
    if isinstance(v, dict):
        return 1 + max([nesting(x) for x in v.values()], default=0)
    if isinstance(v, list):
        return 1 + max([nesting(x) for x in v], default=0)
    return 0


def outer_whitespace(doc: bytes) -> bool:
    """Whether a VALID document holds whitespace outside its strings."""
    inside = escaped = False
    for v in doc:
        if inside:
            if escaped:
                escaped = False
            elif v == 0x5C:
                escaped = True
            elif v == 0x22:
                inside = False
        elif v == 0x22:
            inside = True
        elif v in b" \t\n\r":
            return True
    return False


CHARS = list("abz09 _-:,[]{}") + ["é", "€", "好", "𝄞", "߿", "퟿", "", "\U0010ffff", '"', "\\", "/", "\b", "\f", "\n", "\r", "\t",
                                  "\x01", "\x1f", "\x7f"]
FLOATS = [0.5, -1.25e-7, 3e20, 1e-05, 123.456, 2.0 ** 70, -0.0, 1.5e300, 5e-324]
INTS = [0, 1, -1, 7, 10, -90, 12345678901234567890, -10 ** 30]


def random_value(rng, depth):
    kind = rng.choice(["str", "int", "float", "lit"] + (["list", "dict"] * 2 if depth > 0 else []))
    if kind == "str":
        return "".join(rng.choice(CHARS) for _ in range(rng.choice([0, 1, 2, 3, 6])))
    if kind == "int":
        return rng.choice(INTS + [rng.randrange(-10 ** 6, 10 ** 6)])
    if kind == "float":
        return rng.choice(FLOATS + [rng.uniform(-1e3, 1e3), rng.random() * 10.0 ** rng.randint(-30, 30)])
    if kind == "lit":
        return rng.choice([True, False, None])
    n = rng.choice([0, 0, 1, 2, 3])
    if kind == "list":
        return [random_value(rng, depth - 1) for _ in range(n)]
    return {"".join(rng.choice(CHARS) for _ in range(rng.choice([0, 1, 2, 4]))): random_value(rng, depth - 1) for _ in range(n)}


@functools.lru_cache(maxsize=None)
def values():
    rng = random.Random(8259)
    out = [random_value(rng, d % 7) for d in range(420)]
    assert {nesting(v) for v in out} >= set(range(7)) and any(v == [] for v in out) and any(v == {} for v in out)
    return out


# written by hand: what json.dumps never writes
HAND = [b'"\\/"', b'"\\u00e9\\uD834\\uDD1E\\udead"', b"-0", b"0e0", b"0E+0", b"1.0E-2", b"-0.0e-0", b'{"a":{"a":[[],{}]},"a":null}', b"[[[[[[]]]]]]",
        b"1e999", b'""', b"10", b'"\xf0\x90\x80\x80\xf4\x8f\xbf\xbf\xed\x9f\xbf\xee\x80\x80\xe0\xa0\x80"']
HAND_BAD = [b"", b"01", b"-", b"1.", b".5", b"1e", b"1e+", b"+1", b"[1,]", b"[,1]", b"{,}", b'{"a"}', b'{"a":}', b'{"a":1,}', b"{1:2}", b"tru", b"True",
            b"nul", b"NaN", b"Infinity", b"-Infinity", b"'a'", b'"\x01"', b'"\t"', b'"\\x41"', b'"\\u12g4"', b'"\\"', b'"abc', b"]", b"[1]]", b"[1}",
            b'{"a":1]', b"1 2", b"[1 2]", b'"\xc0\x80"', b'"\xed\xa0\x80"', b'"\xf4\x90\x80\x80"', b'"\xe0\x9f\xbf"', b'"\x80"', b'"\xc3"', b"\xef\xbb\xbf1",
            b"[1,\x00]", b"0x10", b"1_0", b"--1", b"00", b"-01", b"1.e1", b"[\"a\" \"b\"]", b"{\"a\" 1}", b"nulll", b"[]0"]


def test_json_grammar_equals_dumps():
    p, pw = J(False), J(True)
    for v in values():
        for doc in (json.dumps(v, separators=(",", ":"), ensure_ascii=False).encode(), json.dumps(v, separators=(",", ":"), ensure_ascii=True).encode()):
            assert strict_loads(doc)[0] and p.matches(doc) and pw.matches(doc), doc
        for doc in (json.dumps(v, indent=2).encode(), json.dumps(v).encode(), json.dumps(v, indent="\t", ensure_ascii=False).encode(),
                    b" \r\n" + json.dumps(v).encode() + b"\t \n"):
            assert pw.matches(doc), doc
            assert p.matches(doc) == (not outer_whitespace(doc)), doc
    for doc in HAND:
        assert strict_loads(doc)[0] and p.matches(doc) and pw.matches(doc), doc
    for doc in HAND_BAD:
        assert not strict_loads(doc)[0] and not p.matches(doc) and not pw.matches(doc), doc


@pytest.mark.parametrize("whitespace", [False, True], ids=["compact", "whitespace"])
def test_json_grammar_mutations(whitespace):
    """Every document with one byte deleted, one byte duplicated, or truncated at every prefix length: whenever the automaton matches,
    ``json.loads`` accepts; whenever ``json.loads`` accepts (and the nesting is within max_depth) the whitespace automaton matches, and
    the compact one exactly when no whitespace stands outside the strings.  Every proper prefix of a matched document is live."""
    p, pw = J(whitespace), J(True)
    checked = agreed_yes = 0
    for n, v in enumerate(values()):
        doc = (json.dumps(v, indent=1, ensure_ascii=n % 2 == 0) if whitespace else json.dumps(v, separators=(",", ":"), ensure_ascii=n % 2 == 0)).encode()
        if len(doc) > 160:
            doc = doc[:160]                                     # (a long document: its prefix is mutated - invalid to begin with, still compared)
        at = [p.start]
        for k in range(len(doc)):
            at.append(p.step(at[-1], doc[k:k + 1]))
        if p.accepting(at[-1]):
            assert all(c is not None for c in at)               # every proper prefix of a matched document is a live configuration
        mutants = {doc[:k] for k in range(len(doc))}            # truncated at every prefix length
        mutants |= {doc[:k] + doc[k + 1:] for k in range(len(doc))} | {doc[:k + 1] + doc[k:] for k in range(len(doc))}
        for m in mutants:
            k = len(os.path.commonprefix([m, doc]))
            got = p.accepting(p.step(at[k], m[k:]))
            ok, value = strict_loads(m)
            assert not got or ok, m
            if ok:
                assert nesting(value) <= 16 and pw.matches(m), m
                assert got == (whitespace or not outer_whitespace(m)), m
                agreed_yes += 1
            checked += 1
    assert checked > 10000 and agreed_yes > 300, (checked, agreed_yes)      # (a digit deleted or doubled, a truncated number: still JSON)


def test_depth_and_root():
    assert J().matches(b"[" * 16 + b"]" * 16) and not J().matches(b"[" * 17 + b"]" * 17)
    assert J().step(J().start, b"[" * 16) is not None and J().step(J().start, b"[" * 17) is None
    deep = G.json_grammar(max_depth=G.PDA_DEPTH_MAX)
    assert deep.matches(b'{"a":[' * 32 + b"1" + b"]}" * 32) and not deep.matches(b"[" * 65 + b"]" * 65)
    # the window rule is a per-walk option of step(): 33 openers in one walk die under it, 32 and then one more do not
    assert deep.step(deep.start, b"[" * 33, window=G.PDA_LOCAL_MAX) is None
    assert deep.step(deep.step(deep.start, b"[" * 32, window=G.PDA_LOCAL_MAX), b"[", window=G.PDA_LOCAL_MAX) is not None
    assert deep.step(deep.start, b"[" * 20 + b"]" * 20 + b"[" * 30 + b"]" * 30 + b"[" * 33, window=G.PDA_LOCAL_MAX) is None
    low = b"]" * 39 + b","                                      # from 40 open arrays down to one: the lowest depth of the walk is 1
    assert deep.step((1, (1,) * 40), low + b"[" * 32, window=G.PDA_LOCAL_MAX) == (1, (1,) * 33)
    assert deep.step((1, (1,) * 40), low + b"[" * 33, window=G.PDA_LOCAL_MAX) is None and deep.step((1, (1,) * 40), low + b"[" * 33) is not None
    assert J(max_depth=0).matches(b"1") and not J(max_depth=0).matches(b"[]")
    obj, arr = J(root="object"), J(root="array")
    assert obj.matches(b'{"a":[1]}') and obj.matches(b"{}") and not obj.matches(b"[]") and not obj.matches(b"1") and not obj.matches(b'"a"')
    assert arr.matches(b"[{}]") and not arr.matches(b"{}") and not arr.matches(b"1")
    assert J(True, "object").matches(b' {"a" : 1 } ') and not J(True, "object").matches(b" [ ] ")
    for bad in (dict(root="number"), dict(max_depth=65), dict(max_depth=-1)):
        with pytest.raises(ValueError):
            G.json_grammar(**bad)
    assert J().n_syms == 2 and J().n_states <= 64 and J().table.size <= G.GRAMMAR_TABLE_MAX and J().accepting(J().step(J().start, b"[]"))
    assert not J().accepting(J().step(J().start, b"[1")) and not J().accepting(None) and J().step(None, b"1") is None


def test_every_reachable_configuration_can_finish():
    """From every (state, top) reachable within depth 2 some bytes lead to acceptance without a push deeper than the configuration is
    (breadth-first over configurations; a push is refused at max_depth = 2, so finishing never needs one)."""
    for ws in (False, True):
        p = G.json_grammar(whitespace=ws, max_depth=2)
        seen, frontier = {p.start}, [p.start]
        alphabet = [bytes([v]) for v in b' \n"\\/u0a19-+.eE,:[]{}trufalsn\x7f'] + ["é".encode()[:1], "é".encode()[1:], b"\xe0", b"\xa0", b"\xed", b"\xf0",
                                                                                     b"\x90", b"\xf4", b"\xf1", b"\xe1", b"\x80"]
        while frontier:
            nxt = []
            for c in frontier:
                for a in alphabet:
                    d = p.step(c, a)
                    if d is not None and d not in seen:
                        seen.add(d)
                        nxt.append(d)
            frontier = nxt
        assert len({s for s, _ in seen}) == p.n_states           # every state is reached
        can = {c for c in seen if p.accepting(c)}
        changed = True
        while changed:
            changed = False
            for c in seen - can:
                if any(p.step(c, a) in can for a in alphabet):
                    can.add(c)
                    changed = True
        assert can == seen, sorted(seen - can)[:5]


# ---- from_dfa, as_grammar, the caps --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", TG.PATTERNS)
def test_from_dfa_is_the_same_language(pattern):
    dfa = G.compile_regex(pattern)
    pda = G.BytePDA.from_dfa(dfa)
    assert (pda.n_syms, pda.max_depth, pda.n_states, pda.n_classes) == (0, 0, dfa.n_states, dfa.n_classes)
    alphabet = TG.ALPHABET + (["$", "|", "]", "-"] if pattern in ("\\$?a\\|", "[]a]|[b-]") else [])
    for L in range(5):
        for chars in itertools.product(alphabet, repeat=L):
            s = "".join(chars).encode()
            assert pda.matches(s) == dfa.matches(s), (pattern, s)
            c = pda.step(pda.start, s)
            assert (c is None) == (dfa.step(0, s) < 0) and (c is None or c == (dfa.step(0, s), ()))


def test_as_grammar_and_caps():
    d, p = G.compile_regex("[A-D]"), J()
    assert G.as_grammar(d) is d and G.as_grammar(p) is p and isinstance(G.as_grammar("[A-D]"), G.ByteDFA) and G.as_dfa(d) is d
    for bad in (7, None, b"a"):
        with pytest.raises(ValueError):
            G.as_grammar(bad)
    with pytest.raises(ValueError):
        G.as_dfa(p)                                             # as_dfa's callers keep their behaviour
    cls = np.arange(256) % 128
    ok = G.BytePDA(cls, np.full((32, 4, 128), G.PDA_DEAD), np.ones(32), 3, 64)           # exactly at the cap
    assert ok.table.size == G.GRAMMAR_TABLE_MAX == 16384 and (G.PDA_DEPTH_MAX, G.PDA_LOCAL_MAX, G.PDA_SYMS_MAX) == (64, 32, 3)
    with pytest.raises(ValueError, match=r"16512.*16384"):
        G.BytePDA(np.arange(256) % 129, np.full((32, 4, 129), G.PDA_DEAD), np.ones(32), 3, 64)
    with pytest.raises(ValueError, match=r"4096.*4095"):
        G.BytePDA(np.zeros(256), np.full((4096, 1, 1), G.PDA_DEAD), np.ones(4096), 0, 0)
    with pytest.raises(ValueError, match="n_syms 4"):
        G.BytePDA(cls, np.full((2, 5, 128), G.PDA_DEAD), np.ones(2), 4, 8)
    for bad in (dict(max_depth=65), dict(max_depth=-1), dict(n_syms=-1)):
        with pytest.raises(ValueError):
            G.BytePDA(cls, np.full((2, 3, 128), G.PDA_DEAD), np.ones(2), **{"n_syms": 2, "max_depth": 8, **bad})
    with pytest.raises(ValueError):
        G.BytePDA(cls, np.full((2, 2, 128), G.PDA_DEAD), np.ones(2), 2, 8)              # the table's tops do not fit n_syms
    with pytest.raises(ValueError):
        G.BytePDA(np.arange(256), np.full((2, 3, 128), G.PDA_DEAD), np.ones(2), 2, 8)   # a class the table does not have
    assert G.pda_entry(5, G.PDA_PUSH, 2) == 5 | 2 << 12 | 2 << 14 and G.pda_entry(0xFFF, 3, 3) == G.PDA_DEAD


# ---- the host form against the oracle ------------------------------------------------------------------------------------------------------
PIECES = (b'{"', b'":', b'"}]}', b"[[[", b"]]", b"],[", b"1.5e-3,", b"", b"[" * 33, b"[" * 32, b"\xc3", b"\xa9", b"\xe2", b"\x82", b"\xac", b"true", b"null,",
          b'"a"', b"]]]]", b"{}", b'""', b"[]", b"}", b'\\"', b"\\u00", b" ", b"\n  ")
SINGLES = b'[]{},:"0123456789-+.eEtrufalsn\\/bAC xyz'


def pda_vocab(n, seed=0):
    import _grammar_oracle as GO
    return GO.make_vocab(n, seed=seed, singles=SINGLES, alphabet=b'[]{},:"01-.eatrue ABCD', extra=PIECES)


def random_pda_rows(rng, B, N, vocab, choices):
    rows = []
    for _ in range(B):
        pda = rng.choice(choices)
        r = PD.new_row(pda, rng.choice([-1, rng.randrange(N)]), N)
        if pda is not None and rng.random() < 0.6:              # a configuration inside the language: a random walk of allowed ids
            m, config = PD.Machine(r), (0, [])
            for _ in range(rng.randrange(1, 6)):
                ok = sorted(PD.allowed_ids(m, config, vocab, -1, min(N, 120)))
                if not ok:
                    break
                config = m.walk(config[0], config[1], vocab[rng.choice(ok)])
            r["state"], r["depth"] = config[0], len(config[1])
            r["stack"][:len(config[1])] = config[1]
        rows.append(r)
    return rows


@pytest.mark.parametrize("dt", ["f16", "bf16", "f32"])
def test_host_form_equals_oracle(dt):
    rng = random.Random({"f16": 161, "bf16": 611, "f32": 321}[dt])
    g = torch.Generator().manual_seed(7)
    choices = [J(True, max_depth=4), J(False, max_depth=3), J(True, "object", 64), G.BytePDA.from_dfa(G.compile_regex("[A-D]+")),
               G.BytePDA.from_dfa(G.compile_regex("(ab|cd)*e?")), None]
    for case in range(16):
        B, N = rng.choice([1, 3, 4]), rng.choice([9, 60, 140])
        vocab = pda_vocab(rng.choice([N, N, max(1, N - 3), N + 5]), seed=case)
        rows = random_pda_rows(rng, B, N, vocab, choices)
        st = fused_ops.PdaState(B, G.token_byte_table(vocab), "cpu").arm([r["pda"] for r in rows], [r["eos"] for r in rows])
        PD.device_rows(st, rows)
        with_rows = case % 2 == 0
        row_state = [[0, PD.FINISHED if rng.random() < 0.2 else 0] for _ in rows] if with_rows else None
        rs_t = torch.tensor(row_state, dtype=torch.int32) if with_rows else None
        for step in range(4):
            x = (torch.randn(B, N, generator=g) * 3).to(DT[dt])
            bits = to_bits(x)
            tok = None if step == 0 else [rng.choice([rng.randrange(N), rng.randrange(N), -1, N, N + 7, 2 ** 40]) for _ in range(B)]
            for b, r in enumerate(rows):                        # ... more often than not an id the row's configuration survives
                if tok is not None and r["pda"] is not None and r["state"] >= 0 and rng.random() < 0.7:
                    ok = sorted(PD.allowed_ids(PD.Machine(r), (r["state"], r["stack"][:r["depth"]]), vocab, -1, N))
                    long = [i for i in ok if len(vocab[i]) > 1]
                    tok[b] = rng.choice(long if long and rng.random() < 0.7 else ok) if ok else tok[b]
            if step == 3:                                       # ... and corrupt rows: a dead state, a depth out of range, a foreign symbol
                for b, r in enumerate(rows):
                    if r["pda"] is not None and rng.random() < 0.5:
                        kind = rng.choice(["dead", "depth", "symbol", "syms", "maxd"])
                        if kind == "dead":
                            r["state"] = -1
                        elif kind == "depth":
                            r["depth"] = rng.choice([-1, 65, 5])
                        elif kind == "symbol":
                            r["depth"], r["stack"][0:2] = 2, [3, rng.choice([1, 3])]
                        elif kind == "syms":
                            r["n_syms"] = rng.choice([9, -2, 1])
                        else:
                            r["max_depth"] = rng.choice([1000, -5, 1])
                PD.device_rows(st, rows)
            PD.launch(bits, dt, rows, vocab, tok, row_state)
            out = fused_ops.pda_mask(x, st, None if tok is None else torch.tensor(tok, dtype=torch.int64), rs_t)
            assert out is x
            assert np.array_equal(to_bits(x), bits), (dt, case, step)
            PD.assert_rows(st, rows)


def test_host_form_cases():
    vocab = [b"[", b"]", b"1", b",", b"", b"[[", b"]]", b"", b'{"a":', b"}", b"[" * 33, b"[" * 32]
    p = G.json_grammar(max_depth=3)
    st = fused_ops.PdaState(2, G.token_byte_table(vocab), "cpu").arm([p, None], [7, 7])
    allowed = lambda x: [i for i in range(len(vocab)) if not torch.isinf(x[0, i])]
    x = torch.zeros(2, 12)
    fused_ops.pda_mask(x, st)
    assert allowed(x) == [0, 2, 5, 8] and not torch.isinf(x[1]).any() and st.configs() == [(0, ()), (0, ())]
    for fed, want, depth in ((5, [0, 1, 2, 6, 8], 2), (0, [1, 2, 6], 3), (2, [1, 2, 3, 6], 3), (6, [1, 3], 1), (3, [0, 2, 5, 8], 1), (8, [0, 2, 8], 2),
                             (4, [0, 2, 8], 2), (7, [0, 2, 8], 2), (0, [1, 2], 3), (1, [3, 9], 2), (9, [1, 3], 1), (1, [7], 0)):
        x.zero_()
        fused_ops.pda_mask(x, st, torch.tensor([fed, 0]))
        assert allowed(x) == want and st.depth.tolist() == [depth, 0] and st.ticket.tolist() == [0, 0], (fed, allowed(x), st.configs())
    assert p.accepting(st.configs()[0]) and st.stack[0, :3].tolist() == [1, 2, 1]        # what a pop leaves behind is not cleared
    x.zero_()
    fused_ops.pda_mask(x, st, torch.tensor([2, 0]))             # fed "1" behind a complete document: dead - only the end id is left alone
    assert st.states()[0] == -1 and st.configs()[0] is None and allowed(x) == [7]
    deep = fused_ops.PdaState(1, G.token_byte_table(vocab), "cpu").arm([G.json_grammar(max_depth=64)], [7])
    x = torch.zeros(1, 12)
    fused_ops.pda_mask(x, deep)
    assert allowed(x) == [0, 2, 5, 8, 11]                       # the window rule: 32 openers in one token, not 33
    fused_ops.pda_mask(x.zero_(), deep, torch.tensor([11]))
    assert allowed(x) == [0, 1, 2, 5, 6, 8, 11] and deep.depth.tolist() == [32]
    fused_ops.pda_mask(x.zero_(), deep, torch.tensor([11]))
    assert allowed(x) == [1, 2, 6] and deep.depth.tolist() == [64]


def test_argument_errors():
    vocab = G.token_byte_table([b"a", b"b", b"c"])
    p, d = J(), G.compile_regex("a")
    with pytest.raises(ValueError):
        fused_ops.PdaState(0, vocab, "cpu")
    with pytest.raises(ValueError):
        fused_ops.PdaState(1, [b"a"], "cpu")
    st = fused_ops.PdaState(2, vocab, "cpu")
    for bad in (([p], None), ([p, "a"], None), ([p, p], [0]), ([p, p], [0, -2]), ([p, p], [0, "x"])):
        with pytest.raises(ValueError):
            st.arm(*bad)
    st.arm([p, d], [2, None])                                   # a ByteDFA is lifted
    assert st.cfg.tolist() == [[p.n_states, 2, 2, 16], [d.n_states, -1, 0, 0]] and st.active and st.states() == [0, 0]
    assert isinstance(st.pdas[1], G.BytePDA) and not fused_ops.PdaState(2, vocab, "cpu").arm(None).active
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(3), st)
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(1, 3), st)
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(2, 6)[:, ::2], st)
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(1, 3).expand(2, 3), st)
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(2, 3), st, torch.zeros(2, dtype=torch.int32))
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(2, 3), st, row_state=torch.zeros(2, 2))
    with pytest.raises(ValueError):
        fused_ops.pda_mask(torch.zeros(2, 3), fused_ops.GrammarState(2, vocab, "cpu"))


def test_declarations():
    header = open(os.path.join(ROOT, "include", "qlinear_hip.h")).read()
    assert re.search(r"^int qlinear_pda_mask\(", header, re.M)
    assert re.search(r"^#define QLINEAR_ABI_VERSION 3$", header, re.M) and "Still 3: qlinear_pda_mask" in header
    assert "Still 3: qlinear_grammar_mask" in header
    for name, value in (("DEPTH_MAX", fused_ops.PDA_DEPTH_MAX), ("LOCAL_MAX", fused_ops.PDA_LOCAL_MAX), ("SYMS_MAX", fused_ops.PDA_SYMS_MAX)):
        assert re.search(rf"^#define QL_PDA_{name} {value}$", header, re.M)
    assert (fused_ops.PDA_DEPTH_MAX, fused_ops.PDA_LOCAL_MAX, fused_ops.PDA_SYMS_MAX) == (G.PDA_DEPTH_MAX, G.PDA_LOCAL_MAX, G.PDA_SYMS_MAX) == (64, 32, 3)
    assert (PD.TABLE_MAX, PD.STATES_MAX, PD.DEPTH_MAX, PD.LOCAL_MAX, PD.SYMS_MAX) == (16384, 4095, 64, 32, 3)
    assert "qlinear_pda_mask" in _lib.EXPORTS
    makefile = open(os.path.join(ROOT, "chatglm_q_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", makefile, re.M).group(1).split()
    assert "pda_mask.hip" in srcs and os.path.exists(os.path.join(ROOT, "chatglm_q_amd", "csrc", "pda_mask.hip"))


# ---- the tiny model ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_f32():
    return build("f32")


def tiny_vocab(n):
    vocab = pda_vocab(n, seed=11)
    eos = [i for i, t in enumerate(vocab) if not t][1]
    assert eos not in TG.PROMPT and all(eos not in q for q in TG.PROMPTS)
    return vocab, eos


def check_json_row(pda, ids, eos, vocab, state):
    """"accepted": ended on the end id and the bytes parse; "open": the budget ran out on a live configuration."""
    assert ids and eos not in ids[:-1] and all(len(vocab[i]) > 0 for i in ids if i != eos), ids
    text = b"".join(vocab[i] for i in ids if i != eos)
    if ids[-1] == eos:
        assert state == "accepted" and strict_loads(text)[0] and pda.matches(text), text
    else:
        assert state == "open" and pda.step(pda.start, text) is not None, text
    return state


def test_generate_ids_with_a_pda(tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=vocab)
    base = list(dec.generate_ids(TG.PROMPT, max_generated_tokens=6, greedy=True))
    assert dec.last_stats["grammar"] is False and dec._session.gr is None and dec._session.pda is None
    list(dec.generate_ids(TG.PROMPT, max_generated_tokens=3, greedy=True, grammar="[A-D]+"))
    assert dec._session.gr is not None and dec._session.pda is None          # a call without a BytePDA: the DFA path, as before
    seen = set()
    for pda in (J(True, max_depth=4), J(False, "object", 2)):
        for budget in (2, 12):
            for mode in (dict(greedy=True), dict(seed=5), dict(seed=6, top_k=3), dict(seed=7, device_sampler=False)):
                ids = list(dec.generate_ids(TG.PROMPT, max_generated_tokens=budget, grammar=pda, **mode))
                seen.add(check_json_row(pda, ids, eos, vocab, dec.last_stats["grammar_state"]))
                assert dec.last_stats["grammar"] is True and dec._session.pda is not None
    assert seen == {"accepted", "open"}
    assert list(dec.generate_ids(TG.PROMPT, max_generated_tokens=6, greedy=True)) == base            # ... and off again


def test_generate_batch_ids_with_mixed_rows(tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=G.token_byte_table(vocab))
    js = J(True, max_depth=4)
    grammars = [js, None, "[A-D]", J(False, "array", 3)]
    for mode in (dict(greedy=True), dict(seed=[3, 4, 5, 6])):
        plain = dec.generate_batch_ids(TG.PROMPTS, max_generated_tokens=8, **mode)
        assert dec.last_stats["grammar"] is False and (dec._batch_sessions[4][1].pda is None or "seed" in mode)
        got = dec.generate_batch_ids(TG.PROMPTS, max_generated_tokens=8, grammar=grammars, **mode)
        states = dec.last_stats["grammar_state"]
        assert dec.last_stats["grammar"] is True and states[1] is None and got[1] == plain[1]
        check_json_row(js, got[0], eos, vocab, states[0])
        check_json_row(grammars[3], got[3], eos, vocab, states[3])
        TG.check_row("[A-D]", got[2], eos, vocab, states[2])
        # the DFA row through the pushdown launch: the ids of the same row through the DFA launch
        dfa_only = dec.generate_batch_ids(TG.PROMPTS, max_generated_tokens=8, grammar=[None, None, "[A-D]", None], **mode)
        assert dfa_only[2] == got[2]
    sess = dec._batch_sessions[4][1]
    assert sess.pda is not None and sess.gr is not None and not sess.pda_armed
    one = dec.generate_batch_ids([TG.PROMPT], max_generated_tokens=8, greedy=True, grammar=js)
    assert one == [list(dec.generate_ids(TG.PROMPT, max_generated_tokens=8, greedy=True, grammar=js))]


def test_api_argument_errors(tiny_f32):
    model, cfg = tiny_f32
    vocab, eos = tiny_vocab(cfg.vocab_size)
    dec = ChatGLMDecoder(cfg, model, eos_token_id=eos, token_bytes=vocab)
    with pytest.raises(ValueError, match="end token"):
        list(dec.generate_ids(TG.PROMPT, max_generated_tokens=3, greedy=True, grammar=J(), ignore_eos=True))
    with pytest.raises(ValueError, match="min_new_tokens"):
        list(dec.generate_ids(TG.PROMPT, max_generated_tokens=3, greedy=True, grammar=J(), min_new_tokens=2))
    with pytest.raises(ValueError, match="min_new_tokens"):
        dec.generate_batch_ids(TG.PROMPTS, max_generated_tokens=3, greedy=True, grammar=[None, J(), None, None], min_new_tokens=[0, 2, 0, 0])
    with pytest.raises(ValueError, match="byte table"):
        list(ChatGLMDecoder(cfg, model, eos_token_id=eos).generate_ids(TG.PROMPT, max_generated_tokens=3, greedy=True, grammar=J()))
    with pytest.raises(TypeError):
        dec.beam_search_ids(TG.PROMPT, num_beams=2, max_generated_tokens=3, grammar=J())
